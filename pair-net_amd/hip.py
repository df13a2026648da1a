"""ctypes binding of libpairnet_hip.so (include/pairnet_hip.h).

torch is used here only for what the boundary needs from it: device memory
(`Tensor.data_ptr()`) and the current HIP stream.  There is NO fallback: if the
library is missing or a launch fails, a RuntimeError is raised.
"""
import contextlib
import ctypes as C
import os
import threading

import torch

from .build import LIB_PATH

# (tuning aid: PAIRNET_LIB=<path> runs the package against an alternative BUILD of the same
# library -- a kernel variant compiled with a build-time knob, tools/bench_variant.py -- with
# the same ABI check; there is still no fallback)
LIB_PATH = os.environ.get("PAIRNET_LIB") or LIB_PATH

_i32, _i64, _f32, _vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p

GEMM_RELU, GEMM_A_COLMAJOR, GEMM_FORCE_TILE, GEMM_FORCE_SKINNY = 1, 2, 4, 8
GEMM_GELU = 256
GEMM_FORCE_TILE64, GEMM_FORCE_TILE128x64 = 16, 32
GEMM_RELU_AFTER_RES = 128
GEMM_GROUP_MAX = 18       # problems per pn_gemm_group_f32 launch (csrc/gemm.hip)


class GemmDesc(C.Structure):
    _fields_ = [("A", _vp), ("lda", _i64), ("strideA", _i64),
                ("Aadd", _vp), ("ldaadd", _i64), ("aadd_rows", _i32),
                ("aadd_from_col", _i32),
                ("W", _vp), ("ldw", _i64), ("strideW", _i64),
                ("bias", _vp),
                ("Res", _vp), ("ldres", _i64), ("strideRes", _i64),
                ("C", _vp), ("ldc", _i64), ("strideC", _i64),
                ("M", _i32), ("N", _i32), ("K", _i32), ("batch", _i32),
                ("flags", _i32),
                ("splitk_scratch", _vp), ("splitk_scratch_floats", _i64)]


class GemmS3Desc(C.Structure):
    _fields_ = [("A", _vp), ("A2", _vp), ("a2_from_col", _i32),
                ("W", _vp), ("bias", _vp),
                ("M", _i32), ("N", _i32), ("K", _i32), ("relu", _i32),
                ("C", _vp), ("ldc", _i64),
                ("CS", _vp),
                ("CS_pos", _vp), ("pos", _vp), ("pos_rows", _i32),
                ("res_s3", _vp), ("gamma", _vp), ("beta", _vp), ("eps", _f32), ("flags", _i32),
                ("act", _i32), ("res", _vp), ("ldres", _i64)]


class GemmS3FfnDesc(C.Structure):
    _fields_ = [("X", _vp), ("W1", _vp), ("b1", _vp), ("W2", _vp), ("b2", _vp),
                ("M", _i32), ("N", _i32), ("K", _i32), ("F", _i32), ("act", _i32),
                ("C", _vp), ("ldc", _i64),
                ("CS", _vp),
                ("CS_pos", _vp), ("pos", _vp), ("pos_rows", _i32),
                ("res_s3", _vp), ("gamma", _vp), ("beta", _vp), ("eps", _f32)]


class GemmS3RowsDesc(C.Structure):
    _fields_ = [("A", _vp), ("lda", _i64),
                ("W", _vp), ("bias", _vp),
                ("M", _i32), ("N", _i32), ("K", _i32), ("act", _i32),
                ("C", _vp), ("ldc", _i64),
                ("CS", _vp),
                ("CS_pos", _vp), ("pos", _vp), ("pos_rows", _i32),
                ("res_s3", _vp), ("gamma", _vp), ("beta", _vp), ("eps", _f32)]


_SIGS = {
    "pn_abi_version": (C.c_int, []),
    "pn_s3_bytes": (_i64, [_i32, _i32]),
    "pn_s3_split_f32": (C.c_int, [_vp, _i64, _vp, _i32, _vp, _i32, _i32, _vp]),
    "pn_s3_join_f32": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _vp]),
    "pn_gemm_s3_f32": (C.c_int, [C.POINTER(GemmS3Desc), _vp]),
    "pn_gemm_s3_ffn_f32": (C.c_int, [C.POINTER(GemmS3FfnDesc), _vp]),
    "pn_gemm_s3_rows_ln_f32": (C.c_int, [C.POINTER(GemmS3RowsDesc), _vp]),
    "pn_s3_split2_f32": (C.c_int, [_vp, _i64, _vp, _i32, _vp, _vp, _i32, _i32, _vp]),
    "pn_gemm_f32": (C.c_int, [C.POINTER(GemmDesc), _vp]),
    "pn_gemm_variant": (C.c_int, [C.POINTER(GemmDesc)]),
    "pn_gemm_grid_size": (C.c_int, [C.POINTER(GemmDesc)]),
    "pn_gemm_wgs_per_cu": (C.c_int, []),
    "pn_gemm_group_f32": (C.c_int, [C.POINTER(GemmDesc), C.c_int, _vp]),
    "pn_conv2d_nhwc_f32": (C.c_int, [_vp, _vp, _vp, _vp] + [_i32] * 10 + [_vp]),
    "pn_conv2d_nhwc_ex_f32": (C.c_int, [_vp] * 5 + [_i32] * 10 + [_vp, _i64, _vp]),
    "pn_bottleneck_proj_f32": (C.c_int, [_vp] * 8 + [_i32] * 8 + [_vp, _i64, _vp]),
    "pn_stem7x7s2_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "pn_maxpool3x3s2_nhwc_f32": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "pn_winograd_f23_input_f32": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "pn_winograd_f23_output_f32": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "pn_winograd_f43_input_f32": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "pn_winograd_f43_output_f32": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "pn_layernorm_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _f32, _vp]),
    "pn_layernorm_rows_s3_f32": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _f32, _vp]),
    "pn_layernorm_rows_f32": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _i32, _f32, _vp]),
    "pn_patch_merge_ln_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp]),
    "pn_patch_im2col4_f32": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "pn_window_attention_f32": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64] + [_i32] * 7 +
                                [_f32, _vp]),
    "pn_window_attention_s3_f32": (C.c_int, [_vp, _i64, _vp, _vp, _vp] + [_i32] * 7 + [_f32, _vp]),
    "pn_groupnorm_nblk": (C.c_int, [_i64]),
    "pn_groupnorm_nhwc_f32": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32,
                                        _i32, _f32, _i32, _i64, _i64, _vp]),
    "pn_groupnorm_upadd_nhwc_f32": (C.c_int, [_vp] * 6 + [_i32] * 7 + [_f32, _i64, _i64, _i64, _vp]),
    "pn_l2normalize_f32": (C.c_int, [_vp, _vp, _i64, _i32, _f32, _vp]),
    "pn_ffn_scratch_floats": (_i64, [_i32, _i32]),
    "pn_ffn_ln_f32": (C.c_int, [_vp] * 9 + [_i32, _i32, _i32, _f32, _vp]),
    "pn_ffn_ln2_f32": (C.c_int, [_vp] * 12 + [_i32, _i32, _i32, _f32, _vp]),
    "pn_msda_f32": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i32, _i32, C.POINTER(_i32),
                              C.POINTER(_i32), _vp]),
    "pn_msda_ex_f32": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i32, _i32, C.POINTER(_i32),
                                 C.POINTER(_i32), _i32, _vp]),
    "pn_linear_res_ln_f32": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i64,
                                       _i32, _i32, _i32, _f32, _vp]),
    "pn_gt_mask_prepare_u8": (C.c_int, [_vp, _vp] + [_i32] * 7 + [_vp]),
    "pn_point_sample_f32": (C.c_int, [_vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "pn_mask_match_cost_f32": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32,
                                         _f32, _f32, _f32, _vp]),
    "pn_id_match_cost_f32": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32,
                                       _f32, _f32, _f32, _vp]),
    "pn_ce_mean_f32": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _f32, _vp]),
    "pn_seesaw_mean_f32": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _f32, _f32, _f32, _f32,
                                     _vp]),
    "pn_bce_posw_mean_f32": (C.c_int, [_vp, _vp, _vp, _i64, _f32, _vp]),
    "pn_ce_mean_grad_f32": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _f32, _vp]),
    "pn_seesaw_mean_grad_f32": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _f32, _f32,
                                          _f32, _f32, _vp]),
    "pn_bce_posw_mean_grad_f32": (C.c_int, [_vp, _vp, _vp, _i64, _f32, _vp]),
    "pn_transpose_f32": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp]),
    "pn_colsum_f32": (C.c_int, [_vp, _i64, _vp, _i32, _i32, _i32, _vp, _i64, _vp]),
    "pn_relu_bwd_f32": (C.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "pn_add_periodic_f32": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp]),
    "pn_batch_sum_f32": (C.c_int, [_vp, _vp, _i32, _i64, _i32, _vp]),
    "pn_layernorm256_bwd_f32": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _f32, _vp]),
    "pn_mha_bwd_f32": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64,
                                 _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp]),
    "pn_mha_keysplit_chunk": (C.c_int, []),
    "pn_mha_bwd_keysplit_scratch_floats": (_i64, [_i32, _i32, _i32]),
    "pn_mha_bwd_keysplit_f32": (C.c_int, [_vp, _i64] * 7 + [_vp, _i64, _i32, _i32, _i32, _f32, _vp]),
    "pn_mha_bwd_keysplit_masked_f32": (C.c_int, [_vp, _i64] * 7 + [_vp, _i64, _i32, _i32, _i32, _f32,
                                                                  _vp, _vp, _vp]),
    "pn_scatter_rows_add_f32": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp]),
    "pn_cosine_bwd_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp]),
    "pn_mlearner_last_bwd_data_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "pn_tapcorr1_f32": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "pn_conv_weight_bwd_layout_f32": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "pn_msda_offaw_bwd_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i32, C.POINTER(_i32),
                                        C.POINTER(_i32), _vp]),
    "pn_groupnorm_nhwc_bwd_f32": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _f32, _i64,
                                            _i64, _vp]),
    "pn_winograd_weights_f32": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "pn_conv_wgrad_f32": (C.c_int, [_vp, _vp, _vp] + [_i32] * 11 + [_vp]),
    "pn_dilate2_f32": (C.c_int, [_vp, _vp] + [_i32] * 7 + [_vp]),
    "pn_subsample2_f32": (C.c_int, [_vp, _vp] + [_i32] * 6 + [_vp]),
    "pn_scale_rows_f32": (C.c_int, [_vp, _vp, _i64, _i64, _vp]),
    "pn_dropout_f32": (C.c_int, [_vp, _vp, _vp, _i64, _f32, C.c_uint64, C.c_uint32, C.c_uint32,
                                 C.c_uint32, _vp]),
    "pn_dropout_keep_u8": (C.c_int, [_vp, _i64, _f32, C.c_uint64, C.c_uint32, C.c_uint32,
                                     C.c_uint32, _vp]),
    "pn_layernorm_rows_bwd_f32": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64,
                                            _i32, _f32, _vp]),
    "pn_patch_merge_ln_bwd_f32": (C.c_int, [_vp] * 5 + [_i32] * 5 + [_f32, _i32, _vp]),
    "pn_gelu_f32": (C.c_int, [_vp, _vp, _i64, _vp]),
    "pn_gelu_bwd_f32": (C.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "pn_window_attention_bwd_f32": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp]
                                    + [_i32] * 7 + [_f32, _vp]),
    "pn_grad_norm_clip_f32": (C.c_int, [_vp, _i64, _f32, _f32, _vp, _vp, _vp]),
    "pn_adamw_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _f32, C.c_double,
                               C.c_double, _f32, _f32, _i32, _vp, _f32, _vp]),
    "pn_adamw_guarded_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _f32,
                                       C.c_double, C.c_double, _f32, _f32, _i32, _vp, _f32, _vp,
                                       _vp]),
    "pn_lsa_f32": (C.c_int, [_vp, _i64, _vp, _i32, _i64, _vp, _vp, _i64, _vp, _vp]),
    "pn_loss_targets": (C.c_int, [_vp] * 6 + [_i64, _i32, _i32, _i32, _i32] + [_vp] * 5),
    "pn_msda_loc_f32": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "pn_msda_bwd_f32": (C.c_int, [_vp, _i64] + [_vp] * 8 + [_i32, _i32, _i32, _i32, _vp]),
    "pn_msda_bwd_det_scratch_bytes": (C.c_int64, [_i32, _i32, _i32, _i32]),
    "pn_msda_bwd_det_f32": (C.c_int, [_vp, _i64] + [_vp] * 9 + [_i64, _i32, _i32, _i32, _i32, _vp]),
    "pn_gather_probe_f32": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp]),
    "pn_sine_pe_f32": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _f32, _vp]),
    "pn_sine_pe_offset_f32": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _f32, _f32, _vp]),
    "pn_bilinear_nhwc_f32": (C.c_int, [_vp, _vp] + [_i32] * 7 + [_i64, _i64, _vp]),
    "pn_bilinear_planar_f32": (C.c_int, [_vp, _vp, _i64] + [_i32] * 4 + [_vp]),
    "pn_bilinear_planar_gt0_u8": (C.c_int, [_vp, _vp, _i64] + [_i32] * 4 + [_vp]),
    "pn_pair_masks_u8": (C.c_int, [_vp, _vp, _vp, _vp] + [_i32] * 6 + [_vp]),
    "pn_mask_pack": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _vp]),
    "pn_mask_pack_stencil": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp]),
    "pn_mask_stencil_gemm_f32": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp] +
                                 [_i32] * 9 + [_vp]),
    "pn_mask_stencil_gather_gemm_f32": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp] +
                                        [_i32] * 9 + [_vp]),
    "pn_bilinear_stencil_rows_f32": (C.c_int, [_vp, _vp] + [_i32] * 6 + [_i64, _i64, _vp]),
    "pn_attn_scratch_floats": (_i64, [_i32, _i32, _i32]),
    "pn_attention_f32": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp,
                                   _i64, _vp, _i32, _i32, _i32, _f32, _vp]),
    "pn_ppn_front_f32": (C.c_int, [_vp] * 6 + [_i32, _i32, _f32, _vp]),
    "pn_mlearner_first_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "pn_mlearner_last_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "pn_topk_pairs": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "pn_topk_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "pn_topk_strided_f32": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "pn_gather_rows_f32": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i64, _vp]),
    "pn_cls_argmax_f32": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "pn_rel_dists_f32": (C.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "pn_softmax_fg_f32": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _vp]),
    "pn_row_argmax_f32": (C.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "pn_triplet_finish": (C.c_int, [_vp] * 9 + [_i32, _i32, _vp]),
    "pn_panoptic_f32": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i64, _vp]),
    "pn_panoptic_state_bytes": (_i64, []),
    "pn_panoptic_device_f32": (C.c_int, [_vp, _vp, _vp] + [_i32] * 6 + [_vp, _vp, _vp, _vp,
                                                                        _i32, _vp]),
    "pn_panoptic_continue_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "pn_resize_kept_f32": (C.c_int, [_vp, _vp, _vp] + [_i32] * 6 + [_vp]),
    "pn_pack_triplets_f32": (C.c_int, [_vp] * 5 + [_i32, _i32, _vp]),
    "pn_copy_stream": (C.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "pn_pack_bool_bits": (C.c_int, [_vp, _vp, _i64, _vp]),
    "pn_unpack_bits_host": (C.c_int, [_vp, _vp, _i64, _i32]),
    "pn_pred_triplets": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "pn_mask_or_rows": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i64, _vp]),
    "pn_triplet_match": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp,
                                   C.c_double, _i32, _i32, _vp, _vp]),
    "pn_triplet_match_boxes": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp,
                                         _vp, _f32, _i32, _i32, _vp, _vp]),
    "pn_eval_record": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "pn_eval_iou_best": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp,
                                   _vp]),
    "pn_eval_iou_best_boxes": (C.c_int, [_vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp]),
    "pn_nogc_triplets_f32": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32,
                                       _vp, _vp, _vp, _vp, _vp, _vp]),
    "pn_pan_masks_u8": (C.c_int, [_vp] * 5 + [_i32] * 3 + [_vp]),
    "pn_preprocess_u8_f32": (C.c_int, [_vp, _i32, _i32, _vp] + [_i32] * 4 + [C.POINTER(_f32),
                                                                            C.POINTER(_f32), _i32, _vp]),
    "pn_augment_image_u8_f32": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _i64] + [_i32] * 5
                                + [C.POINTER(_f32), C.POINTER(_f32), _i32, _vp]),
    "pn_augment_resize_crop_u8": (C.c_int, [_vp] + [_i32] * 7 + [_vp, _i32, _i32, _vp]),
    "pn_augment_masks_u8": (C.c_int, [_vp, _i32, _i32, _vp] + [_i32] * 12 + [_vp, _vp]),
    "pn_pack_mask_bits": (C.c_int, [_vp, _vp, _i64, _i64, _vp]),
    "pn_mask_iou_counts": (C.c_int, [_vp, _i32, _vp, _i32, _i64, _vp, _vp, _vp, _vp]),
    "pn_zero_rows_f32": (C.c_int, [_vp, _vp, _vp, _i32, _i64, _i32, _i64, _i64, _vp]),
    "pn_token_sampling_f32": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, C.POINTER(_i32),
                                        C.POINTER(_i32), _vp]),
    "pn_sine_pe_valid_f32": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _vp]),
    "pn_sigmoid_f32": (C.c_int, [_vp, _vp, _i64, _vp]),
    "pn_box_pos_embed_f32": (C.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "pn_box_sampling_f32": (C.c_int, [_vp, _i64, _vp, _vp, _i32, _vp, _vp, _i64, _i32, _vp]),
    "pn_box_refine_f32": (C.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "pn_query_score_f32": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "pn_box_triplets_f32": (C.c_int, [_vp] * 5 + [_vp, _i32, _i32, _f32, _f32, C.POINTER(_f32),
                                                _i32, _vp]),
    "pn_uniform_f32": (C.c_int, [_vp, _i64, _i32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32,
                                 C.c_uint32, _vp]),
    "pn_seg_targets": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _i64, _i64, _i32, _i32, _i32, _i32,
                                 _i64, _vp, _vp, _vp, _vp, _vp]),
    "pn_uncertain_points_f32": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp,
                                          _i32, _i32, _i32, _vp, _vp, _vp]),
    "pn_point_sample_rows_f32": (C.c_int, [_vp, _i32, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _i32,
                                           _vp]),
    "pn_mask_point_loss_f32": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _f32, _f32, _f32,
                                         _f32, _vp, _vp, _vp, _vp]),
    "pn_point_scatter_scratch_ints": (_i64, [_i64, _i32, _i32, _i32]),
    "pn_point_scatter_grad_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "pn_ce_avg_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp]),
    "pn_ce_avg_grad_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp]),
    "pn_pq_confusion": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp,
                                  _vp]),
    "pn_pq_record": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pn_rel_id_cost_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _i32,
                                     _i32, _i32, _f32, _f32, _f32, _vp]),
    "pn_rel_targets": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32,
                                 _vp, _vp, _vp, _vp]),
    "pn_id_ce_f32": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _f32, _f32, _vp,
                               _vp, _vp, _vp, _vp]),
    "pn_box_match_cost_f32": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _i64,
                                        _i32, _i32, _i32] + [_f32] * 7 + [_vp]),
    "pn_mask_grad_kslice": (C.c_int, []),
    "pn_mask_embed_grad_scratch_floats": (_i64, [_i32, _i64]),
    "pn_mask_embed_grad_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i64, _vp, _i64,
                                         _vp, _vp]),
    "pn_mask_feature_grad_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i64, _i64, _vp,
                                           _vp]),
    "pn_bilinear_nhwc_bwd_f32": (C.c_int, [_vp, _vp] + [_i32] * 7 + [_i64, _i64, _vp]),
    "pn_groupnorm_act_nhwc_bwd_f32": (C.c_int, [_vp] * 10 + [_i32, _i64, _i32, _f32, _i32, _i32,
                                                             _i64, _i64, _vp]),
    "pn_tri_match_cost_f32": (C.c_int, [_vp] * 8 + [_i64, _vp, _i64, _vp] + [_i32] * 10 + [_i64] +
                              [_vp] * 6 + [_i64, _vp, _i64, _vp]),
    "pn_tri_pair_splits": (C.c_int, [_i32, _i32, _i32]),
    "pn_tri_targets": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32,
                                 _i32, _i64] + [_vp] * 7),
    "pn_triplet_heads_bwd_f32": (C.c_int, [_vp] * 14 + [_i32] * 5 + [_vp]),
    "pn_conv2d_grouped_nhwc_f32": (C.c_int, [_vp] * 4 + [_i32] * 9 + [_vp]),
    "pn_train_log_row_f32": (C.c_int, [C.POINTER(_vp), _i32, C.c_uint32, _vp, _vp, _vp, _i32, _i32,
                                       _i32, _vp]),
    "pn_train_log_window_f32": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "pn_det_match_cost_f32": (C.c_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64,
                                        _i64, _i32, _i32] + [_f32] * 7 + [_vp]),
    "pn_det_focal_partials": (_i64, [_i64, _i32, _i32]),
    "pn_det_focal_f32": (C.c_int, [_vp] * 6 + [_i64, _vp, _i64, _i32, _i32, _f32, _f32, _f32, _vp]),
    "pn_det_box_loss_f32": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _vp,
                                      _vp, _vp, _f32, _f32, _f32, _vp]),
    "pn_det_results_f32": (C.c_int, [_vp] * 6 + [_i32] * 5 + [_vp]),
}
EXPORTS = tuple(_SIGS)
ABI_VERSION = 34  # PN_ABI_VERSION of include/pairnet_hip.h these bindings were written for

_lib = None


def lib():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libpairnet_hip.so is missing (%s): run __graft_entry__.build(); "
                "there is no CPU / PyTorch fallback for the Pair-Net hot path" % LIB_PATH)
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        if handle.pn_abi_version() != ABI_VERSION:
            raise RuntimeError("libpairnet_hip.so ABI mismatch; rebuild")
        _lib = handle
    return _lib


class _Reserve(threading.local):
    slots = 0


_reserve = _Reserve()


@contextlib.contextmanager
def reserve_slots(n):
    """Within the block, every persistent tile-kernel launch of THIS thread carries
    PN_GEMM_RESERVE(n): n resident workgroup slots stay free for the kernels of concurrent
    streams.  A per-call hint in the descriptor's flags (include/pairnet_hip.h); nothing
    process-wide is changed, and a captured hipGraph keeps the grids it was captured with."""
    old = _reserve.slots
    _reserve.slots = max(0, int(n)) // 8 * 8
    try:
        yield
    finally:
        _reserve.slots = old


def with_reserve(fn):
    """Method decorator: run under `reserve_slots(self.grid_reserve)`."""
    import functools

    @functools.wraps(fn)
    def wrapper(self, *args, **kw):
        with reserve_slots(getattr(self, "grid_reserve", 0)):
            return fn(self, *args, **kw)
    return wrapper


def _reserve_flag():
    return ((_reserve.slots // 8) & 0x3ff) << 16


def _stream():
    return torch.cuda.current_stream().cuda_stream


def on_device(fn):
    """Method decorator: run with the object's GPU as the current device, so that the
    launches go to THAT device's current stream (a head on cuda:1 called while cuda:0 is
    current would otherwise launch on device 0 against device-1 pointers).  The device is
    `self.device`, or the first device tensor among the arguments before `.to()` was called."""
    import functools

    def first_tensor(objs):
        for o in objs:
            if isinstance(o, torch.Tensor) and o.is_cuda:
                return o.device
            if isinstance(o, (list, tuple)):
                d = first_tensor(o)
                if d is not None:
                    return d
            if isinstance(o, dict):
                d = first_tensor(o.values())
                if d is not None:
                    return d
        return None

    @functools.wraps(fn)
    def wrapper(self, *args, **kw):
        dev = getattr(self, "device", None)
        if dev is None or dev.type != "cuda":
            dev = first_tensor(args)
        if dev is None or dev.type != "cuda" or dev.index == torch.cuda.current_device():
            return fn(self, *args, **kw)
        with torch.cuda.device(dev):
            return fn(self, *args, **kw)
    return wrapper


GEMM_KERNELS = {0: "k_gemm_skinny<A_ROW>", 1: "k_gemm_skinny<A_COL>",
                2: "k_gemm_tile<128,64,64,32,A_ROW>", 3: "k_gemm_tile<128,64,64,32,A_COL>",
                4: "k_gemm_tile<128,128,64,64,A_ROW>", 5: "k_gemm_tile<128,128,64,64,A_COL>",
                6: "k_gemm_tile<64,64,32,32,A_ROW>", 7: "k_gemm_tile<64,64,32,32,A_COL>"}


class KernelTimer:
    """Optional per-launch HIP-event timing (bench.py's roofline leg).  Events are
    recorded on the stream the kernels are launched on (torch's current stream).
    `only`: kernel names to bracket (None = all instrumented launches)."""

    def __init__(self, only=None):
        self.only = set(only) if only else None
        self.records = []   # (name, flops, bytes, start_event, end_event)
        self.meta = []      # per record: problem description (GEMMs: M, N, K, batch) or None

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for name, flops, nbytes, s, e in self.records:
            a = agg.setdefault(name, dict(launches=0, ms=0.0, flops=0.0, bytes=0.0))
            a["launches"] += 1
            a["ms"] += s.elapsed_time(e)
            a["flops"] += flops
            a["bytes"] += nbytes
        return agg


TIMER = None


def _launch(name, flops, nbytes, fn, meta=None):
    t = TIMER
    if t is None or (t.only is not None and name not in t.only):
        return fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    r = fn()
    e.record()
    t.records.append((name, flops, nbytes, s, e))
    t.meta.append(meta)
    return r


def _ptr(t, dtype=torch.float32):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("pairnet_hip kernels take device tensors (got %s)" % t.device)
    if t.dtype != dtype:
        raise RuntimeError("expected %s, got %s" % (dtype, t.dtype))
    return t.data_ptr()


def _check(code, what):
    if code != 0:
        raise RuntimeError("%s failed: %s" % (
            what, "argument contract violated" if code == -1 else "hipError %d" % code))


def _rowmajor(t):
    """(rows, ld) of a 2-D view whose last dim is contiguous."""
    assert t.dim() == 2 and t.stride(1) == 1, (t.shape, t.stride())
    return t.shape[0], t.stride(0)


def gemm_desc(A, W, Cout, *, M, N, K, lda, ldw, ldc, bias=None, aadd=None, ldaadd=0,
              aadd_rows=0, aadd_from_col=0, res=None, ldres=0, batch=1, sA=0, sW=0, sC=0,
              sRes=0, relu=False, colmajor=False, force=None, into=None,
              relu_after=False, scratch=None, gelu=False, ksplit=0):
    """Fill a pn_gemm_desc; tensors only supply base pointers."""
    d = into if into is not None else GemmDesc()
    d.A, d.lda, d.strideA = _ptr(A), lda, sA
    d.Aadd, d.ldaadd, d.aadd_rows, d.aadd_from_col = _ptr(aadd), ldaadd, aadd_rows, aadd_from_col
    d.W, d.ldw, d.strideW = _ptr(W), ldw, sW
    d.bias = _ptr(bias)
    d.Res, d.ldres, d.strideRes = _ptr(res), ldres, sRes
    d.C, d.ldc, d.strideC = _ptr(Cout), ldc, sC
    d.M, d.N, d.K, d.batch = M, N, K, batch
    d.flags = (GEMM_RELU if relu else 0) | (GEMM_A_COLMAJOR if colmajor else 0) | \
        {None: 0, "tile": GEMM_FORCE_TILE, "skinny": GEMM_FORCE_SKINNY, "tile64": 16,
         "tile128x64": 32}[force] | _reserve_flag() | ((ksplit & 31) << 26) | \
        (GEMM_RELU_AFTER_RES if relu_after else 0) | (GEMM_GELU if gelu else 0)
    d.splitk_scratch = _ptr(scratch)
    d.splitk_scratch_floats = scratch.numel() if scratch is not None else 0
    return d


def gemm(A, W, Cout, **kw):
    """Raw pn_gemm_f32 call."""
    d = gemm_desc(A, W, Cout, **kw)
    if TIMER is None:
        _check(lib().pn_gemm_f32(C.byref(d), _stream()), "pn_gemm_f32")
        return
    name = GEMM_KERNELS[lib().pn_gemm_variant(C.byref(d))]
    # every operand of the fused op once: A, W, C, and where present the residual read by the
    # epilogue and the row-periodic addend on A (positional encodings)
    nbytes = 4.0 * d.batch * (d.M * d.K + d.N * d.K + d.M * d.N)
    if d.Res:
        nbytes += 4.0 * d.batch * d.M * d.N
    if d.Aadd:
        nbytes += 4.0 * min(d.aadd_rows, d.M) * d.K
    _check(_launch(name, 2.0 * d.M * d.N * d.K * d.batch, nbytes,
                   lambda: lib().pn_gemm_f32(C.byref(d), _stream()),
                   meta=(d.M, d.N, d.K, d.batch, bool(d.splitk_scratch))), "pn_gemm_f32")


def gemm_group(problems):
    """`problems`: list of kwargs dicts for gemm_desc (+ 'A','W','C'), <= 16, row-major:
    one launch of the grouped (persistent 64x64 tile) kernel."""
    n = len(problems)
    arr = (GemmDesc * n)()
    flops = nbytes = 0.0
    for i, pr in enumerate(problems):
        pr = dict(pr)
        d = gemm_desc(pr.pop("A"), pr.pop("W"), pr.pop("C"), into=arr[i], **pr)
        flops += 2.0 * d.M * d.N * d.K * d.batch
        nbytes += 4.0 * d.batch * (d.M * d.K + d.N * d.K + d.M * d.N)
    _check(_launch("k_gemm_group", flops, nbytes,
                   lambda: lib().pn_gemm_group_f32(arr, n, _stream())), "pn_gemm_group_f32")


def linear(x, weight, bias, out, *, aadd=None, aadd_from_col=0, res=None, relu=False,
           force=None, relu_after=False, scratch=None, gelu=False):
    """out = act((x + aadd[row % len(aadd)]) @ weight.T + bias) + res on 2-D views
    (aadd only feeds output columns >= aadd_from_col)."""
    M, lda = _rowmajor(x)
    N, ldw = _rowmajor(weight)
    Mo, ldc = _rowmajor(out)
    assert Mo == M and out.shape[1] == N and weight.shape[1] == x.shape[1]
    kw = {}
    if aadd is not None:
        ra, lda2 = _rowmajor(aadd)
        kw.update(aadd=aadd, ldaadd=lda2, aadd_rows=ra, aadd_from_col=aadd_from_col)
    if res is not None:
        rr, ldr = _rowmajor(res)
        assert rr == M
        kw.update(res=res, ldres=ldr)
    gemm(x, weight, out, M=M, N=N, K=x.shape[1], lda=lda, ldw=ldw, ldc=ldc, bias=bias,
         relu=relu, force=force, relu_after=relu_after, scratch=scratch, gelu=gelu,
         **kw)


def conv2d_nhwc(x, wp, bias, out, B, H, W, Cin, Cout, KH, KW, pad, relu, big_tile=False,
                tile=None):
    """tile: None (library default: 64x64), "128x64" or "128" (sweeps)."""
    tflag = {None: 0, "128": GEMM_FORCE_TILE, "128x64": GEMM_FORCE_TILE128x64}[tile]
    name = ("k_gemm_tile<128,64,64,32,A_CONV>" if tile == "128x64" else
            "k_gemm_tile<128,128,64,64,A_CONV>" if tile == "128" else
            "k_gemm_tile<64,64,32,32,A_CONV>")
    flops = 2.0 * B * H * W * Cout * KH * KW * Cin
    nbytes = 4.0 * (B * H * W * (Cin + Cout) + Cout * KH * KW * Cin)
    _check(_launch(name, flops, nbytes, lambda: lib().pn_conv2d_nhwc_f32(
        _ptr(x), _ptr(wp), _ptr(bias), _ptr(out), B, H, W, Cin, Cout, KH, KW, pad, int(relu),
        (GEMM_FORCE_TILE if big_tile else 0) | tflag | _reserve_flag(),
        _stream())), "pn_conv2d_nhwc_f32")


def conv2d_ex(x, wp, bias, res, out, B, H, W, Cin, Cout, KH, KW, stride, pad, relu=False,
              relu_after=False, scratch=None, tile=None, ksplit=0):
    """General channel-last convolution (stride, residual, ReLU before / after it).  tile: None
    (64x64), "128x64" or "128"; ksplit: PN_GEMM_KSPLIT(n) (0: the library's own choice)."""
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    flops = 2.0 * B * Ho * Wo * Cout * KH * KW * Cin
    nbytes = 4.0 * (B * (H * W * Cin + Ho * Wo * Cout * (2 if res is not None else 1))
                    + Cout * KH * KW * Cin)
    flags = (GEMM_RELU if relu else 0) | (GEMM_RELU_AFTER_RES if relu_after else 0) | \
        {None: 0, "128": GEMM_FORCE_TILE, "128x64": GEMM_FORCE_TILE128x64}[tile] | \
        ((ksplit & 31) << 26) | _reserve_flag()
    _check(_launch("k_gemm_tile<64,64,32,32,A_CONV>", flops, nbytes,
                   lambda: lib().pn_conv2d_nhwc_ex_f32(
                       _ptr(x), _ptr(wp), _ptr(bias), _ptr(res), _ptr(out), B, H, W, Cin, Cout,
                       KH, KW, stride, pad, flags, _ptr(scratch),
                       scratch.numel() if scratch is not None else 0, _stream())),
           "pn_conv2d_nhwc_ex_f32")


def conv3x3_grouped(x, wg, bias, out, B, H, W, G, Cg, stride, relu=False, kh=3, kw=3, flags=0):
    """Grouped 3x3 convolution, pad 1, channel-last (pn_conv2d_grouped_nhwc_f32): x
    [B,H,W,G*Cg], wg [G,Cg,9*Cg] ((ky, kx, ci) rows), out [B,Ho,Wo,G*Cg].  `kh`, `kw`, `flags`
    are passed through as they are (the library refuses anything but 3, 3 and PN_GEMM_RELU)."""
    Ho, Wo = (H - 1) // max(stride, 1) + 1, (W - 1) // max(stride, 1) + 1
    flops = 2.0 * B * Ho * Wo * G * Cg * kh * kw * Cg
    nbytes = 4.0 * (B * (H * W + Ho * Wo) * G * Cg + G * Cg * kh * kw * Cg)
    _check(_launch("k_conv3x3_grouped<%d,%d>" % (Cg, stride), flops, nbytes,
                   lambda: lib().pn_conv2d_grouped_nhwc_f32(
                       _ptr(x), _ptr(wg), _ptr(bias), _ptr(out), B, H, W, G, Cg, kh, kw, stride,
                       (GEMM_RELU if relu else 0) | flags, _stream())),
           "pn_conv2d_grouped_nhwc_f32")


def bottleneck_proj(x, wsc, bsc, t2, w3, b3, idt, out, B, H, W, Cin, planes, stride,
                    scratch=None):
    """out = relu(conv3(t2) + shortcut(x)) of a stage's first bottleneck in one launch
    (pn_bottleneck_proj_f32); `idt` is the intermediate of the two-launch form the library
    takes where its split-K / skinny rules apply."""
    Cout = w3.shape[0]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    flops = 2.0 * B * Ho * Wo * Cout * (Cin + planes)
    nbytes = 4.0 * (B * (Ho * Wo * (Cin + planes + Cout)) + Cout * (Cin + planes))
    _check(_launch("k_gemm_proj", flops, nbytes,
                   lambda: lib().pn_bottleneck_proj_f32(
                       _ptr(x), _ptr(wsc), _ptr(bsc), _ptr(t2), _ptr(w3), _ptr(b3), _ptr(idt),
                       _ptr(out), B, H, W, Cin, planes, Cout, stride, _reserve_flag(),
                       _ptr(scratch), scratch.numel() if scratch is not None else 0, _stream())),
           "pn_bottleneck_proj_f32")


def stem7x7s2(img, wp, bias, out, B, H, W):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    _check(_launch("k_stem7x7s2", 2.0 * B * Ho * Wo * 64 * 147,
                   4.0 * B * (3 * H * W + Ho * Wo * 64),
                   lambda: lib().pn_stem7x7s2_f32(_ptr(img), _ptr(wp), _ptr(bias), _ptr(out), B,
                                                  H, W, _reserve_flag(), _stream())),
           "pn_stem7x7s2_f32")


def maxpool3x3s2(x, out, B, H, W, Cc):
    _check(lib().pn_maxpool3x3s2_nhwc_f32(_ptr(x), _ptr(out), B, H, W, Cc, _stream()),
           "pn_maxpool3x3s2_nhwc_f32")


def _winograd_weights_dev(w, form):
    """The device form of the two transforms below (one HIP kernel, no BLAS call)."""
    w = w.contiguous()
    co, ci = w.shape[0], w.shape[1]
    U = torch.empty((16 if form == 2 else 36), co, ci, device=w.device, dtype=torch.float32)
    _check(lib().pn_winograd_weights_f32(_ptr(w), _ptr(U), co, ci, form, _stream()),
           "pn_winograd_weights_f32")
    return U


def winograd_weights(w):
    """conv weight [Cout][Cin][3][3] (fp32) -> U [16][Cout][Cin] = G g G^T.  Device tensors go
    through `pn_winograd_weights_f32`; host tensors (tests, tools) through the einsum below."""
    if w.is_cuda:
        return _winograd_weights_dev(w, 2)
    G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]],
                     dtype=torch.float64, device=w.device)
    U = torch.einsum("ik,ockl,jl->ijoc", G, w.double(), G)
    return U.reshape(16, w.shape[0], w.shape[1]).float().contiguous()


def winograd43_weights(w):
    """conv weight [Cout][Cin][3][3] -> U [36][Cout][Cin] = G g G^T for F(4x4, 3x3)."""
    if w.is_cuda:
        return _winograd_weights_dev(w, 4)
    G = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6],
                      [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
                     dtype=torch.float64, device=w.device)
    U = torch.einsum("ik,ockl,jl->ijoc", G, w.double(), G)
    return U.reshape(36, w.shape[0], w.shape[1]).float().contiguous()


def conv3x3_winograd43(x, U, bias, out, V, Mbuf, B, H, W, Cin, Cout, relu):
    """F(4x4,3x3) form; V / Mbuf: 36 * B*ceil(H/4)*ceil(W/4) * Cin / Cout floats."""
    T = B * ((H + 3) // 4) * ((W + 3) // 4)
    _check(lib().pn_winograd_f43_input_f32(_ptr(x), _ptr(V), B, H, W, Cin, _stream()),
           "pn_winograd_f43_input_f32")
    gemm(V, U, Mbuf, M=T, N=Cout, K=Cin, lda=Cin, ldw=Cin, ldc=Cout, batch=36, sA=T * Cin,
         sW=Cout * Cin, sC=T * Cout)
    _check(lib().pn_winograd_f43_output_f32(_ptr(Mbuf), _ptr(bias), _ptr(out), B, H, W, Cout,
                                            int(relu), _stream()), "pn_winograd_f43_output_f32")


def conv3x3_winograd(x, U, bias, out, V, Mbuf, B, H, W, Cin, Cout, relu):
    """3x3 pad-1 stride-1 convolution as Winograd F(2x2,3x3): input transform, one batched
    GEMM over the 16 transform positions, output transform.  V / Mbuf: scratch of
    16 * B*ceil(H/2)*ceil(W/2) * Cin / Cout floats."""
    T = B * ((H + 1) // 2) * ((W + 1) // 2)
    _check(lib().pn_winograd_f23_input_f32(_ptr(x), _ptr(V), B, H, W, Cin, _stream()),
           "pn_winograd_f23_input_f32")
    gemm(V, U, Mbuf, M=T, N=Cout, K=Cin, lda=Cin, ldw=Cin, ldc=Cout, batch=16, sA=T * Cin,
         sW=Cout * Cin, sC=T * Cout)
    _check(lib().pn_winograd_f23_output_f32(_ptr(Mbuf), _ptr(bias), _ptr(out), B, H, W, Cout,
                                            int(relu), _stream()), "pn_winograd_f23_output_f32")


def layernorm(x, gamma, beta, out, eps=1e-5):
    rows = x.numel() // 256
    _check(lib().pn_layernorm_f32(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(out), rows, 256,
                                  eps, _stream()), "pn_layernorm_f32")


def linear_res_ln(x, weight, bias, res, gamma, beta, out, eps=1e-5):
    """out = LayerNorm(res + x @ weight.T + bias) * gamma + beta, 256 output columns, one
    launch (csrc/gemm_ln.hip); bit for bit linear(..., res=res) followed by layernorm()."""
    M, ldx = _rowmajor(x)
    N, ldw = _rowmajor(weight)
    Mr, ldr = _rowmajor(res)
    Mo, ldo = _rowmajor(out)
    K = x.shape[1]
    assert Mr == M and Mo == M and N == 256 and weight.shape[1] == K
    # operands of the fused op once each: x, W, residual in, normalised rows out
    nbytes = 4.0 * (M * K + N * K + 2 * M * N)
    _check(_launch("k_gemm_rowln", 2.0 * M * N * K, nbytes,
                   lambda: lib().pn_linear_res_ln_f32(_ptr(x), ldx, _ptr(weight), ldw, _ptr(bias),
                                                      _ptr(res), ldr, _ptr(gamma), _ptr(beta),
                                                      _ptr(out), ldo, M, N, K, eps, _stream()),
                   meta=(M, N, K, 1, False)), "pn_linear_res_ln_f32")


def s3_floats(rows, K):
    """Size of the S3 operand of a [rows x K] matrix, in float32 elements (arena carving)."""
    return ((rows + 31) // 32) * (K // 16) * 768


def pos8(pos):
    """The `out + pos` table of gemm_s3 in the order its epilogue reads ("P8",
    csrc/gemm_s3.hip): [rows / 32][cols / 16][2][32][8] from fp32 rows [rows][cols]."""
    rows, cols = pos.shape
    rb = (rows + 31) // 32
    p = pos.new_zeros(rb * 32, cols)
    p[:rows] = pos
    return p.view(rb, 32, cols // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous()


def s3_split(x, out, add=None, out_add=None):
    """out (an S3 buffer, any dtype, >= s3_floats(rows, K) * 4 bytes) = split(x + add[row % len(add)])
    for 2-D fp32 rows x: the three-bf16-plane operand format of gemm_s3 (include/pairnet_hip.h).
    With `out_add`: out = split(x) and out_add = split(x + add) from one read of x (one launch,
    bit for bit the two separate calls)."""
    rows, ld = _rowmajor(x)
    K = x.shape[1]
    assert out.numel() * out.element_size() >= s3_floats(rows, K) * 4
    ar = 0
    if add is not None:
        ar, lda = _rowmajor(add)
        assert lda == K and add.shape[1] == K
    if out_add is not None:
        assert add is not None
        assert out_add.numel() * out_add.element_size() >= s3_floats(rows, K) * 4
        _check(_launch("k_s3_split2", 0.0, 16.0 * rows * K,
                       lambda: lib().pn_s3_split2_f32(_ptr(x), ld, _ptr(add), ar, _ptr(out),
                                                      _ptr(out_add), rows, K, _stream())),
               "pn_s3_split2_f32")
        return
    _check(_launch("k_s3_split", 0.0, 10.0 * rows * K,
                   lambda: lib().pn_s3_split_f32(_ptr(x), ld, _ptr(add), ar, _ptr(out), rows, K,
                                                 _stream())), "pn_s3_split_f32")


def s3_join(s3, out):
    """out (2-D fp32 rows) = the exact fp32 values of the S3 operand."""
    rows, ld = _rowmajor(out)
    _check(_launch("k_s3_join", 0.0, 10.0 * rows * out.shape[1],
                   lambda: lib().pn_s3_join_f32(_ptr(s3), _ptr(out), ld, rows, out.shape[1],
                                                _stream())), "pn_s3_join_f32")


def gemm_s3(a, w, M, N, K, *, bias=None, relu=False, out=None, out_s3=None, out_s3_pos=None,
            pos=None, a2=None, a2_from_col=0, res_s3=None, gamma=None, beta=None, eps=1e-5,
            tile96=False, tile192=False, gelu=False, res=None, relu_after=False):
    """fp32 GEMM on the bf16 matrix pipe from pre-split operands (csrc/gemm_s3.hip):
    out = act(a @ w.T + bias), or LayerNorm(a @ w.T + bias + res) * gamma + beta (N == 256).
    a, a2, w, res_s3, out_s3, out_s3_pos are S3 buffers; out is 2-D fp32 rows."""
    d = GemmS3Desc()
    d.A, d.A2, d.a2_from_col = _ptr(a), _ptr(a2), a2_from_col
    d.W, d.bias = _ptr(w), _ptr(bias)
    d.M, d.N, d.K, d.relu = M, N, K, int(relu)
    if out is not None:
        Mo, ldc = _rowmajor(out)
        assert Mo == M and out.shape[1] >= N
        d.C, d.ldc = _ptr(out), ldc
    d.CS, d.CS_pos = _ptr(out_s3), _ptr(out_s3_pos)
    if out_s3_pos is not None:
        # pos: the table in P8 order (pos8()), pos_rows its true row count
        pos, pr = pos
        assert pos.numel() == (pr + 31) // 32 * 32 * N
        d.pos, d.pos_rows = _ptr(pos), pr
    d.res_s3, d.gamma, d.beta, d.eps = _ptr(res_s3), _ptr(gamma), _ptr(beta), eps
    d.flags = (1 if tile96 else 0) | (2 if tile192 else 0)     # PN_GEMM_S3_TILE96 / _TILE192
    d.act = 3 if relu_after else 2 if gelu else 0
    if res is not None:              # fp32 rows added after the activation (a block's shortcut)
        Mr, ldr = _rowmajor(res)
        assert Mr == M and res.shape[1] >= N
        d.res, d.ldres = _ptr(res), ldr
    nbytes = 6.0 * (M * K + N * K) + (4.0 * M * N if out is not None else 0.0) + \
        6.0 * M * N * ((out_s3 is not None) + (out_s3_pos is not None) + (res_s3 is not None))
    name = "k_gemm_s3<ln>" if gamma is not None else "k_gemm_s3"    # (both tile forms)
    _check(_launch(name, 2.0 * M * N * K, nbytes, lambda: lib().pn_gemm_s3_f32(C.byref(d), _stream()),
                   meta=(M, N, K, 1, False)), "pn_gemm_s3_f32")


def gemm_s3_ffn(x, w1, w2, M, N, K, F, *, b1=None, b2=None, res_s3=None, gamma=None, beta=None,
                eps=1e-5, out=None, out_s3=None, out_s3_pos=None, pos=None, gelu=False):
    """The encoder's FFN as one launch (csrc/gemm_s3.hip, k_gemm_s3_ffn):
    LayerNorm(relu(x @ w1.T + b1) @ w2.T + b2 + res) * gamma + beta, bit for bit the
    gemm_s3(relu=True, out_s3=hidden) -> gemm_s3(hidden, res_s3=, gamma=, beta=) pair without the
    hidden rows in memory.  x [M x K], w1 [F x K], w2 [N x F], res_s3, out_s3, out_s3_pos are S3
    buffers; out is 2-D fp32 rows.  K == N == 256, F % 256 == 0, ReLU and a LayerNorm only: the
    library refuses the rest."""
    d = GemmS3FfnDesc()
    d.X, d.W1, d.b1, d.W2, d.b2 = _ptr(x), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2)
    d.M, d.N, d.K, d.F, d.act = M, N, K, F, 2 if gelu else 1
    if out is not None:
        Mo, ldc = _rowmajor(out)
        assert Mo == M and out.shape[1] >= N
        d.C, d.ldc = _ptr(out), ldc
    d.CS, d.CS_pos = _ptr(out_s3), _ptr(out_s3_pos)
    if out_s3_pos is not None:
        pos, pr = pos                # the table in P8 order (pos8()), pos_rows its true row count
        assert pos.numel() == (pr + 31) // 32 * 32 * N
        d.pos, d.pos_rows = _ptr(pos), pr
    d.res_s3, d.gamma, d.beta, d.eps = _ptr(res_s3), _ptr(gamma), _ptr(beta), eps
    nbytes = 6.0 * (M * K + 2 * F * K) + (4.0 * M * N if out is not None else 0.0) + \
        6.0 * M * N * ((out_s3 is not None) + (out_s3_pos is not None) + (res_s3 is not None))
    _check(_launch("k_gemm_s3_ffn", 2.0 * M * F * (K + N), nbytes,
                   lambda: lib().pn_gemm_s3_ffn_f32(C.byref(d), _stream()),
                   meta=(M, N, F, 1, False)), "pn_gemm_s3_ffn_f32")


def gemm_s3_rows_ln(a, w, M, N, K, *, bias=None, res_s3=None, gamma=None, beta=None, eps=1e-5,
                    out=None, out_s3=None, out_s3_pos=None, pos=None):
    """gemm_s3's LayerNorm form reading its activation operand as fp32 rows (csrc/gemm_s3.hip,
    k_gemm_s3_rows): LayerNorm(a @ w.T + bias + res) * gamma + beta, bit for bit the
    s3_split(a) -> gemm_s3(res_s3=, gamma=, beta=) pair without the split pass and its buffer.
    a is 2-D fp32 rows [M x K] (row pitch % 4 == 0); w, res_s3, out_s3, out_s3_pos are S3 buffers;
    out is 2-D fp32 rows.  N == 256, K % 32 == 0 and a LayerNorm only: the library refuses the rest."""
    d = GemmS3RowsDesc()
    Ma, lda = _rowmajor(a)
    assert Ma >= M
    d.A, d.lda = _ptr(a), lda
    d.W, d.bias = _ptr(w), _ptr(bias)
    d.M, d.N, d.K, d.act = M, N, K, 0
    if out is not None:
        Mo, ldc = _rowmajor(out)
        assert Mo == M and out.shape[1] >= N
        d.C, d.ldc = _ptr(out), ldc
    d.CS, d.CS_pos = _ptr(out_s3), _ptr(out_s3_pos)
    if out_s3_pos is not None:
        pos, pr = pos                # the table in P8 order (pos8()), pos_rows its true row count
        assert pos.numel() == (pr + 31) // 32 * 32 * N
        d.pos, d.pos_rows = _ptr(pos), pr
    d.res_s3, d.gamma, d.beta, d.eps = _ptr(res_s3), _ptr(gamma), _ptr(beta), eps
    nbytes = 4.0 * M * K + 6.0 * N * K + (4.0 * M * N if out is not None else 0.0) + \
        6.0 * M * N * ((out_s3 is not None) + (out_s3_pos is not None) + (res_s3 is not None))
    _check(_launch("k_gemm_s3_rows", 2.0 * M * N * K, nbytes,
                   lambda: lib().pn_gemm_s3_rows_ln_f32(C.byref(d), _stream()),
                   meta=(M, N, K, 1, False)), "pn_gemm_s3_rows_ln_f32")


def layernorm_rows(x, gamma, beta, out, eps=1e-5):
    """LayerNorm over the last dim of 2-D row views (any C % 4 == 0, C <= 3072)."""
    rows, ldx = _rowmajor(x)
    ro, ldo = _rowmajor(out)
    assert ro == rows and out.shape[1] == x.shape[1]
    _check(_launch("k_ln_rows", 0.0, 8.0 * rows * x.shape[1],
                   lambda: lib().pn_layernorm_rows_f32(_ptr(x), ldx, _ptr(gamma), _ptr(beta),
                                                       _ptr(out), ldo, rows, x.shape[1], eps,
                                                       _stream())), "pn_layernorm_rows_f32")


def layernorm_rows_s3(x, gamma, beta, out_s3, eps=1e-5):
    """LayerNorm over the last dim of 2-D rows, written as an S3 operand (three bf16 planes:
    gemm_s3's A) instead of fp32 rows; C % 16 == 0."""
    rows, ldx = _rowmajor(x)
    Cc = x.shape[1]
    assert out_s3.numel() >= s3_floats(rows, Cc)
    _check(_launch("k_ln_rows<s3>", 0.0, 10.0 * rows * Cc,
                   lambda: lib().pn_layernorm_rows_s3_f32(_ptr(x), ldx, _ptr(gamma), _ptr(beta),
                                                          _ptr(out_s3), rows, Cc, eps, _stream())),
           "pn_layernorm_rows_s3_f32")


def patch_merge_ln(x, gamma, beta, out, B, H, W, C, eps=1e-5):
    """x [B][H*W][C] -> out [B][ceil(H/2)*ceil(W/2)][4C] = LayerNorm of the 2x2 neighbourhoods
    concatenated neighbour-major ((row*2+col)*C + c); gamma / beta in that order."""
    _check(_launch("k_ln_rows<merge>", 0.0, 8.0 * B * H * W * C,
                   lambda: lib().pn_patch_merge_ln_f32(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(out),
                                                       B, H, W, C, eps, _stream())),
           "pn_patch_merge_ln_f32")


def patch_im2col4(img, out, B, H, W):
    """NCHW RGB image -> [B*ceil(H/4)*ceil(W/4)][64] rows of 4x4 patches (c*16+ky*4+kx, 48
    columns + 16 zeros); pixels beyond H / W read as zero."""
    _check(_launch("k_patch_im2col", 0.0, 4.0 * B * H * W * 3 * 2.4,
                   lambda: lib().pn_patch_im2col4_f32(_ptr(img), _ptr(out), B, H, W, _stream())),
           "pn_patch_im2col4_f32")


def window_attention(qkv, qkv_bias, table, out, B, H, W, C, heads, ws, shift):
    """(Shifted-)window attention on the [B*H*W][3C] qkv rows -> out [B*H*W][C];
    `table` is the relative position bias table transposed to [heads][(2ws-1)^2]."""
    n, ldq = _rowmajor(qkv)
    no, ldo = _rowmajor(out)
    assert n == no == B * H * W and qkv.shape[1] == 3 * C
    hp, wp = -(-H // ws) * ws, -(-W // ws) * ws
    flops = 4.0 * B * hp * wp * (ws * ws) * C
    _check(_launch("k_window_attn", flops, 16.0 * n * C,
                   lambda: lib().pn_window_attention_f32(_ptr(qkv), ldq, _ptr(qkv_bias),
                                                         _ptr(table), _ptr(out), ldo, B, H, W, C,
                                                         heads, ws, shift, 32 ** -0.5, _stream())),
           "pn_window_attention_f32")


def window_attention_s3(qkv, qkv_bias, table, out_s3, B, H, W, C, heads, ws, shift):
    """window_attention() with the output as an S3 operand buffer (gemm_s3's A) instead of rows."""
    n, ldq = _rowmajor(qkv)
    assert n == B * H * W and qkv.shape[1] == 3 * C and out_s3.numel() >= s3_floats(n, C)
    hp, wp = -(-H // ws) * ws, -(-W // ws) * ws
    flops = 4.0 * B * hp * wp * (ws * ws) * C
    _check(_launch("k_window_attn", flops, 18.0 * n * C,
                   lambda: lib().pn_window_attention_s3_f32(_ptr(qkv), ldq, _ptr(qkv_bias), _ptr(table),
                                                            _ptr(out_s3), B, H, W, C, heads, ws, shift,
                                                            32 ** -0.5, _stream())),
           "pn_window_attention_s3_f32")


def groupnorm_nblk(hw):
    return lib().pn_groupnorm_nblk(hw)


def groupnorm_nhwc(x, gamma, beta, out, partials, B, HW, G, relu, x_bstride, y_bstride,
                   eps=1e-5):
    _check(lib().pn_groupnorm_nhwc_f32(
        _ptr(x), _ptr(gamma), _ptr(beta), _ptr(out), _ptr(partials, torch.float64), B, HW,
        256, G, eps, int(relu), x_bstride, y_bstride, _stream()), "pn_groupnorm_nhwc_f32")


def groupnorm_upadd_nhwc(x, gamma, beta, out, partials, coarse, B, H, W, hc, wc, G, x_bstride,
                         y_bstride, coarse_bstride, eps=1e-5):
    """out = GroupNorm(x) + bilinear-up(coarse) in one pass (pn_groupnorm_upadd_nhwc_f32)."""
    _check(lib().pn_groupnorm_upadd_nhwc_f32(
        _ptr(x), _ptr(gamma), _ptr(beta), _ptr(out), _ptr(partials, torch.float64), _ptr(coarse),
        B, H, W, hc, wc, 256, G, eps, x_bstride, y_bstride, coarse_bstride, _stream()),
        "pn_groupnorm_upadd_nhwc_f32")


def ffn_scratch_floats(M, hidden):
    return lib().pn_ffn_scratch_floats(M, hidden)


def ffn_ln(x, W1, b1, W2, b2, gamma, beta, out, scratch, M, hidden, eps=1e-5, post=None):
    """post = (gamma2, beta2, out2): a second LayerNorm of the result into out2."""
    g2, b2n, y2 = post if post is not None else (None, None, None)
    _check(_launch("k_ffn_partial+k_reduce_ln", 4.0 * M * 256 * hidden,
                   4.0 * (2 * 256 * hidden + 2 * M * 256),
                   lambda: lib().pn_ffn_ln2_f32(_ptr(x), _ptr(W1), _ptr(b1), _ptr(W2), _ptr(b2),
                                                _ptr(gamma), _ptr(beta), _ptr(out), _ptr(g2),
                                                _ptr(b2n), _ptr(y2), _ptr(scratch), M, 256, hidden,
                                                eps, _stream())), "pn_ffn_ln2_f32")


def l2normalize(x, out, eps=1e-12):
    _check(lib().pn_l2normalize_f32(_ptr(x), _ptr(out), x.numel() // 256, 256, eps,
                                    _stream()), "pn_l2normalize_f32")


MSDA_PERSISTENT, MSDA_PERSISTENT_BATCHED, MSDA_LOW_OCCUPANCY = 1, 2, 4   # PN_MSDA_* launch forms (A/B)


MSDA_S3_OUT = 8     # PN_MSDA_S3_OUT


def msda(value, ld_value, offaw, ld_offaw, out, B, shapes, flags=0, s3_out=False):
    """`s3_out`: `out` is an S3 operand buffer [B * N x 256] (gemm_s3's A) instead of fp32 rows."""
    if s3_out:
        flags |= MSDA_S3_OUT
    L = len(shapes)
    hs = (_i32 * L)(*[s[0] for s in shapes])
    ws = (_i32 * L)(*[s[1] for s in shapes])
    n = sum(h * w for h, w in shapes)
    # algorithmic bytes: value read + offsets/logits read + output write
    nbytes = 4.0 * B * n * (256 + 8 * L * 4 * 3 + 256)
    _check(_launch("k_msda", 2.0 * B * n * 8 * L * 4 * 4 * 32 * 2, nbytes,
                   lambda: lib().pn_msda_ex_f32(_ptr(value), ld_value, _ptr(offaw), ld_offaw,
                                                _ptr(out), B, L, hs, ws, flags, _stream())),
           "pn_msda_ex_f32")


def msda_loc(value, ld_value, spatial_shapes, level_start_index, loc, aw, out, B, N, Nq, L):
    nbytes = 4.0 * B * (N * 256 + Nq * (8 * L * 4 * 3 + 256))
    _check(_launch("k_msda_loc", 2.0 * B * Nq * 8 * L * 4 * 4 * 32 * 2, nbytes,
                   lambda: lib().pn_msda_loc_f32(_ptr(value), ld_value,
                                                 _ptr(spatial_shapes, torch.int64),
                                                 _ptr(level_start_index, torch.int64), _ptr(loc),
                                                 _ptr(aw), _ptr(out), B, N, Nq, L, _stream())),
           "pn_msda_loc_f32")


def msda_bwd(value, ld_value, spatial_shapes, level_start_index, loc, aw, grad_out, grad_value,
             grad_loc, grad_aw, B, N, Nq, L):
    _check(lib().pn_msda_bwd_f32(_ptr(value), ld_value, _ptr(spatial_shapes, torch.int64),
                                 _ptr(level_start_index, torch.int64), _ptr(loc), _ptr(aw),
                                 _ptr(grad_out), _ptr(grad_value), _ptr(grad_loc), _ptr(grad_aw),
                                 B, N, Nq, L, _stream()), "pn_msda_bwd_f32")


def msda_bwd_det_scratch_bytes(B, N, Nq, L):
    """Bytes of scratch pn_msda_bwd_det_f32 needs at these sizes (0: sizes it refuses)."""
    return int(lib().pn_msda_bwd_det_scratch_bytes(B, N, Nq, L))


def msda_bwd_det(value, ld_value, spatial_shapes, level_start_index, loc, aw, grad_out, grad_value,
                 grad_loc, grad_aw, B, N, Nq, L, scratch=None):
    """msda_bwd with a bitwise reproducible grad_value (no float atomics; csrc/msda_grad.hip).
    `scratch`: a torch.uint8 device tensor of at least msda_bwd_det_scratch_bytes(B, N, Nq, L)
    bytes, contents arbitrary; None allocates one."""
    if scratch is None:
        scratch = torch.empty(max(msda_bwd_det_scratch_bytes(B, N, Nq, L), 16), dtype=torch.uint8,
                              device=value.device)
    _check(lib().pn_msda_bwd_det_f32(_ptr(value), ld_value, _ptr(spatial_shapes, torch.int64),
                                     _ptr(level_start_index, torch.int64), _ptr(loc), _ptr(aw),
                                     _ptr(grad_out), _ptr(grad_value), _ptr(grad_loc),
                                     _ptr(grad_aw), _ptr(scratch, torch.uint8), scratch.numel(),
                                     B, N, Nq, L, _stream()), "pn_msda_bwd_det_f32")


def gather_probe(lines, idx, out, workgroups, line_mask):
    _check(lib().pn_gather_probe_f32(_ptr(lines), _ptr(idx, torch.int32), _ptr(out), workgroups,
                                     line_mask, _stream()), "pn_gather_probe_f32")


def sine_pe(out, add, h, w, C_=256, temperature=10000.0, offset=0.0, valid=None):
    """valid = (valid_h, valid_w) of a padded map (default: the whole map)."""
    vh, vw = valid if valid is not None else (h, w)
    _check(lib().pn_sine_pe_valid_f32(_ptr(out), _ptr(add), h, w, vh, vw, C_, temperature, offset,
                                      _stream()), "pn_sine_pe_valid_f32")


def bilinear_nhwc(x, out, B, hi, wi, ho, wo, Cc, accumulate, in_bstride, out_bstride):
    _check(lib().pn_bilinear_nhwc_f32(_ptr(x), _ptr(out), B, hi, wi, ho, wo, Cc,
                                      int(accumulate), in_bstride, out_bstride, _stream()),
           "pn_bilinear_nhwc_f32")


def bilinear_planar(x, out, P, hi, wi, ho, wo):
    _check(lib().pn_bilinear_planar_f32(_ptr(x), _ptr(out), P, hi, wi, ho, wo, _stream()),
           "pn_bilinear_planar_f32")


def bilinear_planar_gt0(x, out, P, hi, wi, ho, wo):
    _check(lib().pn_bilinear_planar_gt0_u8(_ptr(x), _ptr(out, torch.uint8), P, hi, wi, ho,
                                           wo, _stream()), "pn_bilinear_planar_gt0_u8")


def mask_pack(logits, bits, rowall, R, Nk):
    _check(lib().pn_mask_pack(_ptr(logits), _ptr(bits, torch.int32),
                              _ptr(rowall, torch.int32), R, Nk, _stream()), "pn_mask_pack")


def mask_pack_stencil(logits4, bits, rowall, R, hi, wi, ho, wo):
    _check(lib().pn_mask_pack_stencil(_ptr(logits4), _ptr(bits, torch.int32),
                                      _ptr(rowall, torch.int32), R, hi, wi, ho, wo, _stream()),
           "pn_mask_pack_stencil")


def mask_stencil_gemm(me, rows, bits, rowall, B, Q, hi, wi, ho, wo, K=256):
    """bits / rowall of one layer's attention mask from the mask embedding `me` [B*Q, K] and the
    level's stencil rows [B, 4*ho*wo, K] in one launch (csrc/gemm.hip k_gemm_stencil)."""
    Nk = ho * wo
    _check(_launch("k_gemm_stencil", 2.0 * B * Q * 4 * Nk * K,
                   4.0 * B * (Q * K + 4 * Nk * K) + B * Q * Nk / 8.0,
                   lambda: lib().pn_mask_stencil_gemm_f32(
                       _ptr(me), me.stride(0), Q * me.stride(0), _ptr(rows), rows.stride(-2),
                       rows.stride(0) if rows.dim() == 3 else 4 * Nk * rows.stride(-2),
                       _ptr(bits, torch.int32), _ptr(rowall, torch.int32), B, Q, Nk, K, hi, wi,
                       ho, wo, _reserve_flag(), _stream()),
                   meta=(Q, 4 * Nk, K, B, False)), "pn_mask_stencil_gemm_f32")


def mask_stencil_gather_gemm(me, mf, bits, rowall, B, Q, hi, wi, ho, wo, K=256):
    """mask_stencil_gemm reading the stencil rows in place from the mask feature `mf`
    [B, hi*wi, K] (csrc/gemm.hip k_gemm_stencil_gather)."""
    Nk = ho * wo
    _check(_launch("k_gemm_stencil_gather", 2.0 * B * Q * 4 * Nk * K,
                   4.0 * B * (Q * K + 4 * Nk * K) + B * Q * Nk / 8.0,
                   lambda: lib().pn_mask_stencil_gather_gemm_f32(
                       _ptr(me), me.stride(0), Q * me.stride(0), _ptr(mf), mf.stride(-2),
                       mf.stride(0) if mf.dim() == 3 else hi * wi * mf.stride(-2),
                       _ptr(bits, torch.int32), _ptr(rowall, torch.int32), B, Q, Nk, K, hi, wi,
                       ho, wo, _reserve_flag(), _stream()),
                   meta=(Q, 4 * Nk, K, B, False)), "pn_mask_stencil_gather_gemm_f32")


def bilinear_stencil_rows(x, out, B, hi, wi, ho, wo, Cc, in_bstride, out_bstride):
    _check(lib().pn_bilinear_stencil_rows_f32(_ptr(x), _ptr(out), B, hi, wi, ho, wo, Cc,
                                              in_bstride, out_bstride, _stream()),
           "pn_bilinear_stencil_rows_f32")


def attn_scratch_floats(B, Q, Nk):
    return lib().pn_attn_scratch_floats(B, Q, Nk)


def attention(q, ldq, k, ldk, v, ldv, bits, rowall, out, ldo, scratch, B, Q, Nk, scale):
    # QK^T and PV: 2 x (2 * B * 8 heads * Q * Nk * 32) flops; bytes: q, k, v, out rows once
    _check(_launch("k_attn_chunk", 8.0 * B * 8 * Q * Nk * 32 / 2,
                   4.0 * B * 256 * (2 * Q + 2 * Nk),
                   lambda: lib().pn_attention_f32(
                       _ptr(q), ldq, _ptr(k), ldk, _ptr(v), ldv, _ptr(bits, torch.int32),
                       _ptr(rowall, torch.int32), _ptr(out), ldo, _ptr(scratch), B, Q, Nk, scale,
                       _stream())), "pn_attention_f32")


def ppn_front(sub_embed, obj_embed, w1, b1, imp_raw, c1, B, Q, eps=1e-12):
    _check(lib().pn_ppn_front_f32(_ptr(sub_embed), _ptr(obj_embed), _ptr(w1), _ptr(b1),
                                  _ptr(imp_raw), _ptr(c1), B, Q, eps, _stream()),
           "pn_ppn_front_f32")


def mlearner_first(x, w1, b1, out, B, S):
    _check(lib().pn_mlearner_first_f32(_ptr(x), _ptr(w1), _ptr(b1), _ptr(out), B, S, 64,
                                       _stream()), "pn_mlearner_first_f32")


def mlearner_last(x, w3, b3, out, B, S):
    _check(lib().pn_mlearner_last_f32(_ptr(x), _ptr(w3), _ptr(b3), _ptr(out), B, S, 64,
                                      _stream()), "pn_mlearner_last_f32")


def topk_pairs(scores, idx, sub, obj, B, Q, k, pair=None):
    _check(lib().pn_topk_pairs(_ptr(scores), _ptr(idx, torch.int64), _ptr(sub, torch.int64),
                               _ptr(obj, torch.int64), _ptr(pair, torch.int64), B, Q, k,
                               _stream()), "pn_topk_pairs")


def topk(scores, idx, quot, rem, B, n, div, k):
    _check(lib().pn_topk_f32(_ptr(scores), _ptr(idx, torch.int64), _ptr(quot, torch.int64),
                             _ptr(rem, torch.int64), B, n, div, k, _stream()), "pn_topk_f32")


def topk_strided(scores, elem_stride, row_stride, idx, quot, rem, B, n, div, k):
    _check(lib().pn_topk_strided_f32(_ptr(scores), elem_stride, row_stride, _ptr(idx, torch.int64),
                                     _ptr(quot, torch.int64), _ptr(rem, torch.int64), B, n, div,
                                     k, _stream()), "pn_topk_strided_f32")


def pair_masks(mp, sub_pos, obj_pos, masks, Q, R, hi, wi, ho, wo):
    i64 = torch.int64
    _check(lib().pn_pair_masks_u8(_ptr(mp), _ptr(sub_pos, i64), _ptr(obj_pos, i64),
                                  _ptr(masks, torch.uint8), Q, R, hi, wi, ho, wo, _stream()),
           "pn_pair_masks_u8")


def gather_rows(x, index, out, B, rows_in, rows_out, length):
    _check(lib().pn_gather_rows_f32(_ptr(x), _ptr(index, torch.int64), _ptr(out), B, rows_in,
                                    rows_out, length, _stream()), "pn_gather_rows_f32")


def cls_argmax(logits, label, score, rows, Cc, label_offset=0):
    _check(lib().pn_cls_argmax_f32(_ptr(logits), _ptr(label, torch.int64), _ptr(score), rows,
                                   Cc, label_offset, _stream()), "pn_cls_argmax_f32")


def rel_dists(logits, out, rows, Cc):
    _check(lib().pn_rel_dists_f32(_ptr(logits), _ptr(out), rows, Cc, _stream()),
           "pn_rel_dists_f32")


def softmax_fg(logits, probs, fg, rows, Cc):
    _check(lib().pn_softmax_fg_f32(_ptr(logits), _ptr(probs), _ptr(fg), rows, Cc, _stream()),
           "pn_softmax_fg_f32")


def row_argmax(x, idx, rows, n):
    _check(lib().pn_row_argmax_f32(_ptr(x), _ptr(idx, torch.int64), rows, n, _stream()),
           "pn_row_argmax_f32")


def triplet_finish(s_label, o_label, probs, tri, rem, labels, r_labels, r_scores, r_dists, k,
                   Cc):
    i64 = torch.int64
    _check(lib().pn_triplet_finish(_ptr(s_label, i64), _ptr(o_label, i64), _ptr(probs),
                                   _ptr(tri, i64), _ptr(rem, i64), _ptr(labels, i64),
                                   _ptr(r_labels, i64), _ptr(r_scores), _ptr(r_dists), k, Cc,
                                   _stream()),
           "pn_triplet_finish")


def panoptic(masks, labels, remap, seg, area, n, HW):
    _check(lib().pn_panoptic_f32(_ptr(masks), _ptr(labels, torch.int64),
                                 _ptr(remap, torch.int32), _ptr(seg, torch.int64),
                                 _ptr(area, torch.int32), n, HW, _stream()), "pn_panoptic_f32")


# argmax / area-filter rounds enqueued up front.  The reference's loop can take at most
# three: the first round merges duplicate stuff classes into their first occurrence (the
# duplicates end with area 0 and are dropped), the second counts the survivors without the
# merge (so the first occurrence can lose the merged area and fall out), and since from
# then on dropping segments only ever grows the others, the third finds nothing to drop.
PAN_ROUNDS = 4


def panoptic_state_bytes():
    return lib().pn_panoptic_state_bytes()


def panoptic_device(masks, labels, scores, Q, num_classes, hi, wi, ho, wo, state, up, area, seg,
                    rounds=None):
    rounds = PAN_ROUNDS if rounds is None else rounds
    _check(lib().pn_panoptic_device_f32(
        _ptr(masks), _ptr(labels, torch.int64), _ptr(scores), Q, num_classes, hi, wi, ho, wo,
        _ptr(state, torch.uint8), _ptr(up), _ptr(area, torch.int32), _ptr(seg, torch.int64),
        rounds, _stream()), "pn_panoptic_device_f32")


def resize_kept(masks, up, state, Q, hi, wi, ho, wo, form=1):
    _check(lib().pn_resize_kept_f32(_ptr(masks), _ptr(up), _ptr(state, torch.uint8), Q, hi, wi, ho,
                                    wo, form, _stream()), "pn_resize_kept_f32")


def panoptic_continue(state, up, area, seg, ho, wo, rounds=None):
    rounds = PAN_ROUNDS if rounds is None else rounds
    _check(lib().pn_panoptic_continue_f32(
        _ptr(state, torch.uint8), _ptr(up), _ptr(area, torch.int32), _ptr(seg, torch.int64),
        ho, wo, rounds, _stream()), "pn_panoptic_continue_f32")


def pack_triplets(labels, r_dists, sub_pos, obj_pos, rec, R, C1):
    i64 = torch.int64
    _check(lib().pn_pack_triplets_f32(_ptr(labels, i64), _ptr(r_dists), _ptr(sub_pos, i64),
                                      _ptr(obj_pos, i64), _ptr(rec), R, C1, _stream()),
           "pn_pack_triplets_f32")


def copy_stream(src, dst, wgs=16):
    """dst <- src (same dtype / shape, both contiguous); `dst` may be a PINNED host tensor: the
    kernel writes it over PCIe from `wgs` workgroups, on torch's current stream."""
    if src.dtype != dst.dtype or src.numel() != dst.numel() or not (
            src.is_contiguous() and dst.is_contiguous()):
        raise RuntimeError("copy_stream takes contiguous tensors of one dtype and size")
    if not src.is_cuda or not (dst.is_cuda or dst.is_pinned()):
        raise RuntimeError("copy_stream: device source, device or pinned-host destination")
    nbytes = src.numel() * src.element_size()
    if nbytes:
        _check(lib().pn_copy_stream(src.data_ptr(), dst.data_ptr(), nbytes, int(wgs), _stream()),
               "pn_copy_stream")


def pack_bool_bits(src, bits):
    """bits[(n + 7) // 8] uint8 <- the n elements of the bool / uint8 device tensor `src` (byte i
    bit j = element 8 i + j), on torch's current stream."""
    n = src.numel()
    if not src.is_cuda or not bits.is_cuda or src.element_size() != 1 or not src.is_contiguous() \
            or bits.dtype != torch.uint8 or bits.numel() < (n + 7) // 8 or not bits.is_contiguous():
        raise RuntimeError("pack_bool_bits: contiguous 1-byte device source, uint8 device "
                           "destination of (n + 7) // 8 bytes")
    if n:
        _check(lib().pn_pack_bool_bits(src.data_ptr(), bits.data_ptr(), n, _stream()),
               "pn_pack_bool_bits")


def unpack_bits_host(bits, out, threads=4):
    """The host half: `out` (a HOST bool / uint8 tensor of n elements) <- the packed bytes in
    the host tensor `bits` (once their copy has completed).  No GPU call; ctypes drops the GIL
    for its duration."""
    n = out.numel()
    if bits.is_cuda or out.is_cuda or out.element_size() != 1 or bits.dtype != torch.uint8 \
            or not (bits.is_contiguous() and out.is_contiguous()) or bits.numel() < (n + 7) // 8:
        raise RuntimeError("unpack_bits_host: contiguous host tensors, uint8 bits of "
                           "(n + 7) // 8 bytes")
    if n:
        _check(lib().pn_unpack_bits_host(bits.data_ptr(), out.data_ptr(), n, int(threads)),
               "pn_unpack_bits_host")


def preprocess_u8(img, H, W, out, Hn, Wn, Hp, Wp, mean, stdinv, to_rgb):
    """mean / stdinv: 3 host floats each, in OUTPUT channel order."""
    m = (_f32 * 3)(*[float(v) for v in mean])
    s = (_f32 * 3)(*[float(v) for v in stdinv])
    _check(lib().pn_preprocess_u8_f32(_ptr(img, torch.uint8), H, W, _ptr(out), Hn, Wn, Hp, Wp,
                                      m, s, int(to_rgb), _stream()), "pn_preprocess_u8_f32")


# ---- train-time input pipeline (csrc/augment.hip) ----
def augment_image(img, H, W, flip, batch, slot, Hn, Wn, mean, stdinv, to_rgb):
    """img [H][W][3] uint8 -> image `slot` of the float32 batch tensor [k][3][Hmax][Wmax]: the last
    Resize of the (flipped) image -> Normalize -> zero Pad up to (Hmax, Wmax)."""
    k, c, Hmax, Wmax = batch.shape
    assert c == 3 and batch.is_contiguous() and 0 <= slot < k and img.is_contiguous()
    m = (_f32 * 3)(*[float(v) for v in mean])
    s = (_f32 * 3)(*[float(v) for v in stdinv])
    _check(lib().pn_augment_image_u8_f32(_ptr(img, torch.uint8), H, W, int(flip), _ptr(batch),
                                         3 * Hmax * Wmax, slot, Hn, Wn, Hmax, Wmax, m, s,
                                         int(to_rgb), _stream()), "pn_augment_image_u8_f32")


def augment_resize_crop(img, H, W, flip, H1, W1, oy, ox, out):
    """out [ch][cw][3] uint8 = the window at (oy, ox) of the [H1][W1] resize of the (flipped)
    img."""
    ch, cw, c = out.shape
    assert c == 3 and out.is_contiguous() and img.is_contiguous()
    _check(lib().pn_augment_resize_crop_u8(_ptr(img, torch.uint8), H, W, int(flip), H1, W1, oy, ox,
                                           _ptr(out, torch.uint8), ch, cw, _stream()),
           "pn_augment_resize_crop_u8")


def augment_masks(png, ids, flip, size1, window, size2, batch_size, out):
    """png [H0][W0][3] uint8 RGB, ids [Gk] int32 -> out [Gk][Hb // 2][Wb // 2] uint8: the masks of
    the kept segments after flip, Resize to `size1`, crop `window` = (oy, ox, ch, cw), Resize to
    `size2`, pad to `batch_size` = (Hb, Wb) and the loss side's nearest half-size resize."""
    H0, W0, c = png.shape
    Gk, (Hb, Wb) = int(ids.shape[0]), batch_size
    assert c == 3 and png.is_contiguous() and out.is_contiguous()
    assert tuple(out.shape) == (Gk, Hb // 2, Wb // 2)
    oy, ox, ch, cw = window
    _check(lib().pn_augment_masks_u8(_ptr(png, torch.uint8), H0, W0, _ptr(ids, torch.int32), Gk,
                                     int(flip), size1[0], size1[1], oy, ox, ch, cw, size2[0],
                                     size2[1], Hb, Wb, _ptr(out, torch.uint8), _stream()),
           "pn_augment_masks_u8")


def pack_mask_bits(masks_u8, words, rows, HW):
    _check(lib().pn_pack_mask_bits(_ptr(masks_u8, torch.uint8), _ptr(words, torch.int64), rows, HW,
                                   _stream()), "pn_pack_mask_bits")


def mask_iou_counts(pred_words, P, gt_words, G, nwords, inter, area_p, area_g):
    _check(lib().pn_mask_iou_counts(_ptr(pred_words, torch.int64), P, _ptr(gt_words, torch.int64),
                                    G, nwords, _ptr(inter, torch.int32),
                                    _ptr(area_p, torch.int32), _ptr(area_g, torch.int32),
                                    _stream()), "pn_mask_iou_counts")


def pred_triplets(labels, r_dists, triplets, scores, R, C1):
    _check(lib().pn_pred_triplets(_ptr(labels, torch.int64), _ptr(r_dists),
                                  _ptr(triplets, torch.int32), _ptr(scores), R, C1, _stream()),
           "pn_pred_triplets")


def mask_or_rows(words, a, b, out, rows, nwords):
    _check(lib().pn_mask_or_rows(_ptr(words, torch.int64), _ptr(a, torch.int32),
                                 _ptr(b, torch.int32), _ptr(out, torch.int64), rows, nwords,
                                 _stream()), "pn_mask_or_rows")


def triplet_match(ptrip, gtrip, P, G, inter, area_p, area_g, ld_inter, ps, po, gs, go, thr, phrdet,
                  ignore_rel, match):
    i32 = torch.int32
    _check(lib().pn_triplet_match(_ptr(ptrip, i32), _ptr(gtrip, i32), P, G, _ptr(inter, i32),
                                  _ptr(area_p, i32), _ptr(area_g, i32), ld_inter, _ptr(ps, i32),
                                  _ptr(po, i32), _ptr(gs, i32), _ptr(go, i32), float(thr),
                                  int(phrdet), int(ignore_rel), _ptr(match, torch.uint8),
                                  _stream()), "pn_triplet_match")


def triplet_match_boxes(ptrip, gtrip, P, G, pbox, ldp, gbox, ldg, ps, po, gs, go, thr, phrdet,
                        ignore_rel, match):
    i32 = torch.int32
    _check(lib().pn_triplet_match_boxes(
        _ptr(ptrip, i32), _ptr(gtrip, i32), P, G, _ptr(pbox), ldp, _ptr(gbox), ldg, _ptr(ps, i32),
        _ptr(po, i32), _ptr(gs, i32), _ptr(go, i32), float(thr), int(phrdet), int(ignore_rel),
        _ptr(match, torch.uint8), _stream()), "pn_triplet_match_boxes")


def eval_record(match_sgdet, match_phrdet, R, G, gt_pred, ks, nk, num_rel, hits, counts):
    """hits [2][nk][num_rel], counts [num_rel] int32 from the two match matrices [R][G]."""
    i32 = torch.int32
    assert hits.numel() == 2 * nk * num_rel and counts.numel() == num_rel
    assert match_sgdet.numel() == R * G and match_phrdet.numel() == R * G
    _check(lib().pn_eval_record(_ptr(match_sgdet, torch.uint8), _ptr(match_phrdet, torch.uint8), R,
                                G, _ptr(gt_pred, i32), _ptr(ks, i32), nk, num_rel, _ptr(hits, i32),
                                _ptr(counts, i32), _stream()), "pn_eval_record")


def eval_iou_best(inter, area_p, area_g, P, n_obj, pred_labels, gt_labels, gs, go, G, valid, best):
    """valid [2][G] uint8, best [2][G] float64 from the counts of mask_iou_counts [P][n_obj]."""
    i32 = torch.int32
    assert inter.numel() == P * n_obj and pred_labels.numel() >= P and gt_labels.numel() >= n_obj
    assert valid.numel() == 2 * G and best.numel() == 2 * G
    _check(lib().pn_eval_iou_best(_ptr(inter, i32), _ptr(area_p, i32), _ptr(area_g, i32), P, n_obj,
                                  _ptr(pred_labels, torch.int64), _ptr(gt_labels, i32),
                                  _ptr(gs, i32), _ptr(go, i32), G, _ptr(valid, torch.uint8),
                                  _ptr(best, torch.float64), _stream()), "pn_eval_iou_best")


def eval_iou_best_boxes(pbox, ldp, pred_labels, R, gbox, ldg, gt_labels, n_obj, valid, best):
    """valid [2][n_obj] uint8, best [2][n_obj] float64: per side and ground-truth OBJECT the best
    box IoU over the predictions of its class (side 0: rows [0, R) of pbox, side 1: [R, 2R))."""
    assert pred_labels.numel() >= 2 * R and gt_labels.numel() >= n_obj
    assert pbox.numel() >= (2 * R - 1) * ldp + 4 and gbox.numel() >= (n_obj - 1) * ldg + 4
    assert valid.numel() == 2 * n_obj and best.numel() == 2 * n_obj
    _check(lib().pn_eval_iou_best_boxes(_ptr(pbox), ldp, _ptr(pred_labels, torch.int64), R,
                                        _ptr(gbox), ldg, _ptr(gt_labels, torch.int32), n_obj,
                                        _ptr(valid, torch.uint8), _ptr(best, torch.float64),
                                        _stream()), "pn_eval_iou_best_boxes")


NOGC_MAX_K = 100       # the reference counts only the best 100 (sgg_metrics.py:306-308)


def nogc_triplets(det, ld, labels, rel_dists, sub_row, obj_row, R, C1, per_row, K, triplets,
                  sub_rows, obj_rows, scores, count):
    """The K best no-graph-constraint triplets of one image (csrc/nogc.hip): triplets [K][3],
    sub_rows / obj_rows [K] int32, scores [K] float32, count [1] int32 = min(K, R * per_row)."""
    i32 = torch.int32
    assert det.numel() >= (2 * R - 1) * ld + 5 and labels.numel() >= 2 * R
    assert rel_dists.numel() == R * C1 and sub_row.numel() >= R and obj_row.numel() >= R
    assert triplets.numel() == 3 * K and sub_rows.numel() == K and obj_rows.numel() == K
    assert scores.numel() == K and count.numel() == 1
    _check(lib().pn_nogc_triplets_f32(_ptr(det), ld, _ptr(labels, torch.int64), _ptr(rel_dists),
                                      _ptr(sub_row, i32), _ptr(obj_row, i32), R, C1, per_row, K,
                                      _ptr(triplets, i32), _ptr(sub_rows, i32),
                                      _ptr(obj_rows, i32), _ptr(scores), _ptr(count, i32),
                                      _stream()), "pn_nogc_triplets_f32")


# ---- panoptic quality (csrc/panoptic_quality.hip) ----
PQ_COLS = 257          # column s = predicted segment s, column 256 = void
PQ_LDS_MAX_G = 61      # largest G whose (G + 1) x 257 table is kept in LDS (64 KB a workgroup)
PQ_PLAIN = 1           # PN_PQ_PLAIN


def pq_confusion(pred, gt_rgb, gt_ids, G, num_classes, instance_offset, N, col_cat, status,
                 flags=0):
    """N [(G + 1)][257], col_cat [256], status [1] int32 (all written whole) from the predicted
    map [H][W] int64 and the ground-truth PNG [H][W][3] uint8; gt_ids [>= G] int32 ascending."""
    i32 = torch.int32
    H, W = int(pred.shape[0]), int(pred.shape[1])
    assert pred.is_contiguous() and gt_rgb.is_contiguous() and tuple(gt_rgb.shape) == (H, W, 3)
    assert N.numel() == (G + 1) * PQ_COLS and col_cat.numel() == 256 and status.numel() == 1
    assert gt_ids.numel() >= max(G, 1)
    _check(lib().pn_pq_confusion(_ptr(pred, torch.int64), _ptr(gt_rgb, torch.uint8), H, W,
                                 _ptr(gt_ids, i32), G, num_classes, instance_offset, flags,
                                 _ptr(N, i32), _ptr(col_cat, i32), _ptr(status, i32), _stream()),
           "pn_pq_confusion")


def pq_record(N, col_cat, gt_cat, gt_crowd, G, num_classes, area_gt, area_pred, match, rec, iou,
              status):
    """(tp, fp, fn) [num_classes][3] int32 and the IoU sums [num_classes] float64 of one image
    from its confusion table; areas [G + 1] / [257] and the matched column per row [G + 1]."""
    i32 = torch.int32
    assert N.numel() == (G + 1) * PQ_COLS and col_cat.numel() == 256 and status.numel() == 1
    assert gt_cat.numel() >= max(G, 1) and gt_crowd.numel() >= max(G, 1)
    assert area_gt.numel() == G + 1 and match.numel() == G + 1 and area_pred.numel() == PQ_COLS
    assert rec.numel() == 3 * num_classes and iou.numel() == num_classes
    _check(lib().pn_pq_record(_ptr(N, i32), _ptr(col_cat, i32), _ptr(gt_cat, i32),
                              _ptr(gt_crowd, i32), G, num_classes, _ptr(area_gt, i32),
                              _ptr(area_pred, i32), _ptr(match, i32), _ptr(rec, i32),
                              _ptr(iou, torch.float64), _ptr(status, i32), _stream()),
           "pn_pq_record")


# ---- box trunk glue (csrc/detr.hip) ----
def zero_rows(x, valid_u8, out, B, rows, Cc, ld=None, per_image=False):
    """valid_u8: [rows] (shared) or, with per_image, [B][rows]; rows of Cc floats at stride ld."""
    _check(lib().pn_zero_rows_f32(_ptr(x), _ptr(valid_u8, torch.uint8), _ptr(out), B, rows, Cc,
                                  Cc if ld is None else ld, rows if per_image else 0, _stream()),
           "pn_zero_rows_f32")


def token_sampling(offaw, ld, valid_ratios, loc, aw, B, shapes):
    L = len(shapes)
    hs = (C.c_int32 * L)(*[h for h, _ in shapes])
    ws = (C.c_int32 * L)(*[w for _, w in shapes])
    _check(lib().pn_token_sampling_f32(_ptr(offaw), ld, _ptr(valid_ratios), _ptr(loc), _ptr(aw), B,
                                       L, hs, ws, _stream()), "pn_token_sampling_f32")


def sigmoid(x, out):
    _check(lib().pn_sigmoid_f32(_ptr(x), _ptr(out), x.numel(), _stream()), "pn_sigmoid_f32")


def box_pos_embed(unact, ref, emb, rows):
    _check(lib().pn_box_pos_embed_f32(_ptr(unact), _ptr(ref), _ptr(emb), rows, _stream()),
           "pn_box_pos_embed_f32")


def box_sampling(offaw, ld, ref, loc, aw, rows, L, valid_ratios=None, rows_per_image=0):
    _check(lib().pn_box_sampling_f32(_ptr(offaw), ld, _ptr(ref), _ptr(valid_ratios),
                                     rows_per_image, _ptr(loc), _ptr(aw), rows, L, _stream()),
           "pn_box_sampling_f32")


def box_refine(delta, ref_in, ref_out, rows):
    _check(lib().pn_box_refine_f32(_ptr(delta), _ptr(ref_in), _ptr(ref_out), rows, _stream()),
           "pn_box_refine_f32")


def query_score(logits, score, B, Nq, Cc):
    _check(lib().pn_query_score_f32(_ptr(logits), _ptr(score), B, Nq, Cc, _stream()),
           "pn_query_score_f32")


def box_triplets(s_cls, o_cls, s_box, o_box, det, labels, R, Cc, img_h, img_w, scale_factor,
                 rescale):
    sf = (C.c_float * 4)(*[float(v) for v in scale_factor])
    _check(lib().pn_box_triplets_f32(_ptr(s_cls), _ptr(o_cls), _ptr(s_box), _ptr(o_box), _ptr(det),
                                     _ptr(labels, torch.int64), R, Cc, float(img_h), float(img_w),
                                     sf, 1 if rescale else 0, _stream()), "pn_box_triplets_f32")


# ---- loss forward (csrc/loss.hip) ----------------------------------------------------------
def pan_masks(rgb, ids, cats, masks, sem=None):
    """rgb [H][W][3] uint8 (RGB panoptic PNG) -> masks [G][H][W] uint8 (`rgb2id(rgb) == ids[g]`)
    and optionally sem [H][W] int32 (category of the last listed owner, 255 = none)."""
    H, W, c = rgb.shape
    G = int(ids.shape[0])
    assert c == 3 and rgb.dtype == torch.uint8 and rgb.is_contiguous()
    assert masks.shape == (G, H, W) and masks.is_contiguous() and masks.dtype in (torch.uint8, torch.bool)
    _check(lib().pn_pan_masks_u8(_ptr(rgb, torch.uint8), _ptr(ids, torch.int32) if G else None,
                                 _ptr(cats, torch.int32) if (G and cats is not None) else None,
                                 _ptr(masks, masks.dtype) if G else None,
                                 _ptr(sem, torch.int32) if sem is not None else None, G, H, W,
                                 _stream()), "pn_pan_masks_u8")


def gt_mask_prepare(masks, out, H, W):
    """masks [G][h][w] bool / uint8 -> out [G][Ho][Wo] uint8: zero-padded to [H][W], then
    nearest-neighbour resized (psgtr.py:126-141)."""
    G, h, w = masks.shape
    assert masks.dtype in (torch.bool, torch.uint8) and out.dtype in (torch.bool, torch.uint8)
    assert out.shape[0] == G and masks.is_contiguous() and out.is_contiguous()
    _check(lib().pn_gt_mask_prepare_u8(_ptr(masks, masks.dtype), _ptr(out, out.dtype), G, h, w, H,
                                       W, out.shape[1], out.shape[2], _stream()),
           "pn_gt_mask_prepare_u8")


def point_sample(maps, pts, out):
    """maps [P][h][w] float32 or bool / uint8; pts [Np][2]; out [P][Np] (mmcv point_sample with
    one point set for all maps)."""
    P, h, w = maps.shape
    u8 = maps.dtype in (torch.bool, torch.uint8)
    _check(lib().pn_point_sample_f32(_ptr(maps, maps.dtype), int(u8), _ptr(pts), _ptr(out), P, h, w,
                                     pts.shape[0], _stream()), "pn_point_sample_f32")


def mask_match_cost(cls, gt_labels, pred_pts, gt_pts, cost, w_cls, w_mask, w_dice, dice_eps):
    Q, ncls = cls.shape
    G, Np = gt_pts.shape
    _check(lib().pn_mask_match_cost_f32(_ptr(cls), ncls, _ptr(gt_labels, torch.int64),
                                        _ptr(pred_pts), _ptr(gt_pts), _ptr(cost), Q, G, Np, w_cls,
                                        w_mask, w_dice, dice_eps, _stream()),
           "pn_mask_match_cost_f32")


def id_match_cost(sub, obj, rel, gt_sub, gt_obj, gt_rel, cost, w_sub, w_obj, w_rel):
    R, ncls = sub.shape
    _check(lib().pn_id_match_cost_f32(_ptr(sub), _ptr(obj), _ptr(rel), ncls, rel.shape[1],
                                      _ptr(gt_sub, torch.int64), _ptr(gt_obj, torch.int64),
                                      _ptr(gt_rel, torch.int64), _ptr(cost), R, gt_sub.shape[0],
                                      w_sub, w_obj, w_rel, _stream()), "pn_id_match_cost_f32")


def ce_mean(logits, target, class_weight, out, loss_weight):
    rows, ld = _rowmajor(logits)
    _check(lib().pn_ce_mean_f32(_ptr(logits), ld, _ptr(target, torch.int64), _ptr(class_weight),
                                _ptr(out), rows, logits.shape[1], loss_weight, _stream()),
           "pn_ce_mean_f32")


def seesaw_mean(logits, target, cum_samples, out, p, q, eps, loss_weight):
    rows, ld = _rowmajor(logits)
    _check(lib().pn_seesaw_mean_f32(_ptr(logits), ld, _ptr(target, torch.int64), _ptr(cum_samples),
                                    _ptr(out), rows, logits.shape[1], p, q, eps, loss_weight,
                                    _stream()), "pn_seesaw_mean_f32")


def ce_mean_grad(logits, target, class_weight, grad, loss_weight):
    rows, ld = _rowmajor(logits)
    rg, ldg = _rowmajor(grad)
    assert rg == rows and grad.shape[1] == logits.shape[1]
    _check(lib().pn_ce_mean_grad_f32(_ptr(logits), ld, _ptr(target, torch.int64), _ptr(class_weight),
                                     _ptr(grad), ldg, rows, logits.shape[1], loss_weight, _stream()),
           "pn_ce_mean_grad_f32")


def seesaw_mean_grad(logits, target, cum_samples, grad, p, q, eps, loss_weight):
    rows, ld = _rowmajor(logits)
    rg, ldg = _rowmajor(grad)
    assert rg == rows and grad.shape[1] == logits.shape[1]
    _check(lib().pn_seesaw_mean_grad_f32(_ptr(logits), ld, _ptr(target, torch.int64),
                                         _ptr(cum_samples), _ptr(grad), ldg, rows, logits.shape[1],
                                         p, q, eps, loss_weight, _stream()), "pn_seesaw_mean_grad_f32")


def bce_posw_mean_grad(logits, target, grad, loss_weight):
    assert grad.numel() == logits.numel()
    _check(lib().pn_bce_posw_mean_grad_f32(_ptr(logits), _ptr(target), _ptr(grad), logits.numel(),
                                           loss_weight, _stream()), "pn_bce_posw_mean_grad_f32")


# ---- backward building blocks of the Pair-Net tail (csrc/grad.hip; composed in grad.py) -----
def transpose(x, out, out_cols=None):
    """out[c][r] = x[r][c]; out [cols][ld >= out_cols], zero-filled from column rows on."""
    rows, ldi = _rowmajor(x)
    cols, ldo = _rowmajor(out)
    assert cols == x.shape[1]
    oc = out.shape[1] if out_cols is None else out_cols
    _check(lib().pn_transpose_f32(_ptr(x), ldi, _ptr(out), ldo, rows, cols, oc, _stream()),
           "pn_transpose_f32")


def colsum(x, out, accumulate=False):
    rows, ld = _rowmajor(x)
    cols = x.shape[1]
    assert out.numel() == cols and out.is_contiguous()
    scratch = torch.empty(min(64, rows // 512) * cols, device=x.device, dtype=torch.float32) \
        if rows >= 1024 else None               # tall matrices: row chunks on many workgroups
    _check(lib().pn_colsum_f32(_ptr(x), ld, _ptr(out), rows, cols, int(accumulate), _ptr(scratch),
                               scratch.numel() if scratch is not None else 0, _stream()),
           "pn_colsum_f32")


def relu_bwd(dy, y, dx):
    assert dy.is_contiguous() and y.is_contiguous() and dx.is_contiguous() and \
        dy.numel() == y.numel() == dx.numel()
    _check(lib().pn_relu_bwd_f32(_ptr(dy), _ptr(y), _ptr(dx), dy.numel(), _stream()),
           "pn_relu_bwd_f32")


def add_periodic(a, b, out):
    """out = a + b tiled over a's leading rows (b.numel() divides a.numel()); out may be a."""
    assert a.is_contiguous() and b.is_contiguous() and out.is_contiguous() and \
        a.numel() == out.numel() and a.numel() % b.numel() == 0
    _check(lib().pn_add_periodic_f32(_ptr(a), _ptr(b), _ptr(out), a.numel(), b.numel(), _stream()),
           "pn_add_periodic_f32")


def batch_sum(x, out, B, accumulate=False):
    assert x.is_contiguous() and out.is_contiguous() and x.numel() == B * out.numel()
    _check(lib().pn_batch_sum_f32(_ptr(x), _ptr(out), B, out.numel(), int(accumulate), _stream()),
           "pn_batch_sum_f32")


def layernorm256_bwd(dy, x, gamma, dx, gxhat, eps=1e-5):
    rows = x.shape[0]
    for t in (dy, x, dx, gxhat):
        assert t.is_contiguous() and tuple(t.shape) == (rows, 256)
    _check(lib().pn_layernorm256_bwd_f32(_ptr(dy), _ptr(x), _ptr(gamma), _ptr(dx), _ptr(gxhat),
                                         rows, eps, _stream()), "pn_layernorm256_bwd_f32")


def mha_bwd_scratch_floats(B, Nq, Nk):
    return 2 * B * 8 * Nq * Nk


def mha_bwd(q, k, v, dout, dq, dk, dv, scratch, B, Nq, Nk, scale, bits=None, rowall=None):
    """q / dout / dq: 2-D views [B*Nq, 256] (any row stride), k / v / dk / dv [B*Nk, 256];
    bits / rowall: the forward's packed boolean mask (pn_mask_pack's outputs) or None."""
    ld = lambda t: _rowmajor(t)[1]
    assert scratch.numel() >= mha_bwd_scratch_floats(B, Nq, Nk)
    _check(lib().pn_mha_bwd_f32(_ptr(q), ld(q), _ptr(k), ld(k), _ptr(v), ld(v), _ptr(dout), ld(dout),
                                _ptr(dq), ld(dq), _ptr(dk), ld(dk), _ptr(dv), ld(dv),
                                _ptr(bits, torch.int32), _ptr(rowall, torch.int32), _ptr(scratch),
                                B, Nq, Nk, scale, _stream()), "pn_mha_bwd_f32")


MHA_KEYSPLIT_CHUNK = 256   # KS_CHUNK of csrc/attn_grad.hip (pn_mha_keysplit_chunk(): checked on use)


def mha_bwd_keysplit_scratch_floats(B, Nq, Nk):
    """B * 8 * Nq * (6 + 32 * chunks): row statistics and per-chunk dq partials."""
    return B * 8 * Nq * (6 + 32 * ((Nk + MHA_KEYSPLIT_CHUNK - 1) // MHA_KEYSPLIT_CHUNK))


def mha_bwd_keysplit(q, k, v, dout, dq, dk, dv, scratch, B, Nq, Nk, scale, bits=None, rowall=None):
    """`mha_bwd` with the keys split across workgroups: the same 2-D views (any row stride).
    Without `bits` / `rowall` the unmasked entry (pn_mha_bwd_keysplit_f32), as always; with either,
    pn_mha_bwd_keysplit_masked_f32 under the forward's packed mask (pn_mask_pack's outputs; one
    without the other is refused by the library)."""
    ld = lambda t: _rowmajor(t)[1]
    L = lib()
    if L.pn_mha_keysplit_chunk() != MHA_KEYSPLIT_CHUNK:
        raise RuntimeError("libpairnet_hip.so: key chunk %d, bindings %d; rebuild"
                           % (L.pn_mha_keysplit_chunk(), MHA_KEYSPLIT_CHUNK))
    if bits is not None or rowall is not None:
        _check(L.pn_mha_bwd_keysplit_masked_f32(
            _ptr(q), ld(q), _ptr(k), ld(k), _ptr(v), ld(v), _ptr(dout), ld(dout), _ptr(dq), ld(dq),
            _ptr(dk), ld(dk), _ptr(dv), ld(dv), _ptr(scratch), scratch.numel(), B, Nq, Nk, scale,
            _ptr(bits, torch.int32), _ptr(rowall, torch.int32), _stream()),
            "pn_mha_bwd_keysplit_masked_f32")
        return
    _check(L.pn_mha_bwd_keysplit_f32(_ptr(q), ld(q), _ptr(k), ld(k), _ptr(v), ld(v), _ptr(dout),
                                     ld(dout), _ptr(dq), ld(dq), _ptr(dk), ld(dk), _ptr(dv),
                                     ld(dv), _ptr(scratch), scratch.numel(),
                                     B, Nq, Nk, scale, _stream()), "pn_mha_bwd_keysplit_f32")


def scatter_rows_add(src, index, out, B, rows_out, slots, length, accumulate=False):
    """src [B * slots, >= length], out [B * rows_out, >= length] (2-D views, free row strides)."""
    (rs, lds), (ro, ldo) = _rowmajor(src), _rowmajor(out)
    assert rs == B * slots and ro == B * rows_out and index.numel() == B * slots
    _check(lib().pn_scatter_rows_add_f32(_ptr(src), lds, _ptr(index, torch.int64), _ptr(out), ldo,
                                         B, rows_out, slots, length, int(accumulate), _stream()),
           "pn_scatter_rows_add_f32")


def cosine_bwd(draw, x, other_hat, dx, B, Q, transposed, eps=1e-12):
    _check(lib().pn_cosine_bwd_f32(_ptr(draw), _ptr(x), _ptr(other_hat), _ptr(dx), B, Q,
                                   int(transposed), eps, _stream()), "pn_cosine_bwd_f32")


def mlearner_last_bwd_data(g, w3, c, dc, B, S):
    _check(lib().pn_mlearner_last_bwd_data_f32(_ptr(g), _ptr(w3), _ptr(c), _ptr(dc), B, S, _stream()),
           "pn_mlearner_last_bwd_data_f32")


def tapcorr1(F, g, part, B, S, sgn):
    assert part.numel() == B * S * 49 * 64
    _check(lib().pn_tapcorr1_f32(_ptr(F), _ptr(g), _ptr(part), B, S, sgn, _stream()),
           "pn_tapcorr1_f32")


def conv_weight_bwd_layout(w, out, Co, T, Ci):
    assert w.numel() == out.numel() == Co * T * Ci
    _check(lib().pn_conv_weight_bwd_layout_f32(_ptr(w), _ptr(out), Co, T, Ci, _stream()),
           "pn_conv_weight_bwd_layout_f32")


def msda_offaw_bwd(grad_loc, grad_aw, aw, d_offaw, shapes):
    """d [offsets | logits] rows (2-D view, free row stride) from pn_msda_bwd_f32's outputs."""
    rows, ld = _rowmajor(d_offaw)
    L = len(shapes)
    hs = (C.c_int32 * L)(*[h for h, _ in shapes])
    ws = (C.c_int32 * L)(*[w for _, w in shapes])
    _check(lib().pn_msda_offaw_bwd_f32(_ptr(grad_loc), _ptr(grad_aw), _ptr(aw), _ptr(d_offaw), ld,
                                       rows, L, hs, ws, _stream()), "pn_msda_offaw_bwd_f32")


def groupnorm_nhwc_bwd(x, dy, gamma, dx, gxhat, stats, B, HW, G, x_bstride, dy_bstride, eps=1e-5):
    _check(lib().pn_groupnorm_nhwc_bwd_f32(_ptr(x), _ptr(dy), _ptr(gamma), _ptr(dx), _ptr(gxhat),
                                           _ptr(stats), B, HW, G, eps, x_bstride, dy_bstride,
                                           _stream()), "pn_groupnorm_nhwc_bwd_f32")


def bilinear_nhwc_bwd(dout, din, B, hi, wi, ho, wo, Cc, accumulate, dout_bstride, din_bstride):
    """Adjoint of `bilinear_nhwc` (an upsampling): din [B][hi*wi][Cc] (+)= T^T dout [B][ho*wo][Cc]."""
    _check(lib().pn_bilinear_nhwc_bwd_f32(_ptr(dout), _ptr(din), B, hi, wi, ho, wo, Cc,
                                          int(accumulate), dout_bstride, din_bstride, _stream()),
           "pn_bilinear_nhwc_bwd_f32")


def groupnorm_act_bwd_scratch(B, HW, G, device):
    """(partials, colpart) of `groupnorm_act_nhwc_bwd` for B images of HW pixels."""
    nblk = groupnorm_nblk(HW)
    return (torch.empty(B * nblk * G * 4, device=device, dtype=torch.float64),
            torch.empty(B * nblk * 512, device=device, dtype=torch.float32))


def groupnorm_act_nhwc_bwd(x, dy, y, gamma, dx, dgamma, dbeta, stats, scratch, B, HW, G, relu,
                           accumulate, x_bstride, dy_bstride, eps=1e-5):
    """GroupNorm (+ReLU, gate from the saved output `y`) backward on the forward's row blocking;
    `scratch` from `groupnorm_act_bwd_scratch`; d gamma / d beta written or, with `accumulate`,
    added into."""
    partials, colpart = scratch
    nblk = groupnorm_nblk(HW)
    assert partials.numel() >= B * nblk * G * 4 and colpart.numel() >= B * nblk * 512
    assert dx.is_contiguous() and dx.numel() == B * HW * 256 and stats.numel() >= B * G * 4
    assert y is None or (y.is_contiguous() and y.numel() == B * HW * 256)
    assert dgamma.is_contiguous() and dbeta.is_contiguous() and dgamma.numel() == dbeta.numel() == 256
    _check(lib().pn_groupnorm_act_nhwc_bwd_f32(
        _ptr(x), _ptr(dy), _ptr(y), _ptr(gamma), _ptr(dx), _ptr(dgamma), _ptr(dbeta), _ptr(stats),
        _ptr(partials, torch.float64), _ptr(colpart), B, HW, G, eps, int(relu), int(accumulate),
        x_bstride, dy_bstride, _stream()), "pn_groupnorm_act_nhwc_bwd_f32")


def conv_wgrad(dY, X, part, B, Hi, Wi, Ho, Wo, Ci, Co, K, stride, pad, rows_per):
    assert part.numel() == B * ((Ho + rows_per - 1) // rows_per) * Co * K * K * Ci
    _check(lib().pn_conv_wgrad_f32(_ptr(dY), _ptr(X), _ptr(part), B, Hi, Wi, Ho, Wo, Ci, Co, K,
                                   stride, pad, rows_per, _stream()), "pn_conv_wgrad_f32")


def dilate2(x, out, B, Hi, Wi, Ho, Wo, Cc, accumulate=False):
    _check(lib().pn_dilate2_f32(_ptr(x), _ptr(out), B, Hi, Wi, Ho, Wo, Cc, int(accumulate),
                                _stream()), "pn_dilate2_f32")


def subsample2(x, out, B, Hi, Wi, Ho, Wo, Cc):
    _check(lib().pn_subsample2_f32(_ptr(x), _ptr(out), B, Hi, Wi, Ho, Wo, Cc, _stream()),
           "pn_subsample2_f32")


def scale_rows(x, s):
    rows = s.numel()
    assert x.is_contiguous() and x.numel() % rows == 0
    _check(lib().pn_scale_rows_f32(_ptr(x), _ptr(s), rows, x.numel() // rows, _stream()),
           "pn_scale_rows_f32")


# ---- the relation decoder's FFN dropout (csrc/dropout.hip; composed in grad.py) ------------------
def dropout(x, out, p, seed, subseq, step, site, res=None):
    """out = x * keep / (1 - p) (+ res); keep: Philox4x32-10 at counter (element / 4, subseq, site,
    step) under key `seed`, regenerated by any later call with the same arguments (the backward
    pass: the same call on the gradient).  out may be x."""
    assert x.is_contiguous() and out.is_contiguous() and x.numel() == out.numel() and \
        (res is None or (res.is_contiguous() and res.numel() == x.numel()))
    _check(lib().pn_dropout_f32(_ptr(x), _ptr(res), _ptr(out), x.numel(), p, seed, subseq, step,
                                site, _stream()), "pn_dropout_f32")


def dropout_keep(n, p, seed, subseq, step, site, device=None):
    """The keep bits `dropout` uses for n elements, as a uint8 tensor (1 = kept)."""
    keep = torch.empty(n, device=device or torch.device("cuda", torch.cuda.current_device()),
                       dtype=torch.uint8)
    _check(lib().pn_dropout_keep_u8(_ptr(keep, torch.uint8), n, p, seed, subseq, step, site,
                                    _stream()), "pn_dropout_keep_u8")
    return keep


# ---- Swin backbone backward (csrc/swin_grad.hip; composed in backbone_grad.py) ---------------
def layernorm_rows_bwd(dy, x, gamma, dx, gxhat, eps=1e-5):
    """LayerNorm backward over 2-D row views of any width C % 4 == 0, C <= 3072, from the saved
    input x: dx, and gxhat = dy * xhat (its column sum is d weight; d bias: column sum of dy)."""
    rows, ldx = _rowmajor(x)
    Cc = x.shape[1]
    (r1, lddy), (r2, lddx), (r3, ldg) = _rowmajor(dy), _rowmajor(dx), _rowmajor(gxhat)
    assert r1 == r2 == r3 == rows and dy.shape[1] == dx.shape[1] == gxhat.shape[1] == Cc
    _check(lib().pn_layernorm_rows_bwd_f32(_ptr(dy), lddy, _ptr(x), ldx, _ptr(gamma), _ptr(dx), lddx,
                                           _ptr(gxhat), ldg, rows, Cc, eps, _stream()),
           "pn_layernorm_rows_bwd_f32")


def patch_merge_ln_bwd_nblocks(B, H, W):
    """Workgroups of patch_merge_ln_bwd = rows of its d gamma / d beta partials: four merged rows
    per workgroup at a time, at most 512 workgroups (2048 waves: two per SIMD of the chip)."""
    rows = B * (-(-H // 2)) * (-(-W // 2))
    return max(1, min(-(-rows // 4), 512))


def patch_merge_ln_bwd(dy, x, gamma, dx, part, B, H, W, C, eps=1e-5, accumulate=False):
    """Backward of patch_merge_ln(): dy [B*ceil(H/2)*ceil(W/2)][4C], the saved map x [B*H*W][C],
    gamma [4C] neighbour-major -> dx [B*H*W][C] (every row written once; `accumulate`: added to)
    and part [patch_merge_ln_bwd_nblocks(B, H, W)][2][4C] (column-sum it: d gamma | d beta)."""
    rows = B * (-(-H // 2)) * (-(-W // 2))
    nblk = patch_merge_ln_bwd_nblocks(B, H, W)
    for t in (dy, x, gamma, dx, part):
        assert t.is_contiguous()
    assert dy.numel() == rows * 4 * C and x.numel() == dx.numel() == B * H * W * C
    assert gamma.numel() == 4 * C and part.numel() == nblk * 8 * C
    nbytes = 4.0 * (2 * rows * 4 * C + (2 + bool(accumulate)) * B * H * W * C)
    _check(_launch("k_patch_merge_ln_bwd", 20.0 * rows * 4 * C, nbytes,
                   lambda: lib().pn_patch_merge_ln_bwd_f32(
                       _ptr(dy), _ptr(x), _ptr(gamma), _ptr(dx), _ptr(part), nblk, B, H, W, C, eps,
                       int(bool(accumulate)), _stream())), "pn_patch_merge_ln_bwd_f32")


def gelu(x, out):
    """out = exact (erf) GELU of x (contiguous, same size)."""
    assert x.is_contiguous() and out.is_contiguous() and x.numel() == out.numel()
    _check(lib().pn_gelu_f32(_ptr(x), _ptr(out), x.numel(), _stream()), "pn_gelu_f32")


def gelu_bwd(dy, x, dx):
    """dx = dy * GELU'(x), x the saved pre-activation; dx may alias dy."""
    assert dy.is_contiguous() and x.is_contiguous() and dx.is_contiguous() and \
        dy.numel() == x.numel() == dx.numel()
    _check(lib().pn_gelu_bwd_f32(_ptr(dy), _ptr(x), _ptr(dx), dy.numel(), _stream()),
           "pn_gelu_bwd_f32")


def window_partials_rows(B, H, W, ws):
    """Rows of window_attention_bwd's bias-table partials: B * windows of the padded map."""
    return B * (-(-H // ws)) * (-(-W // ws))


def window_attention_bwd(qkv, qkv_bias, table, dout, dqkv, dtable_part, B, H, W, C, heads, ws,
                         shift, out=None):
    """Backward of window_attention(): qkv [B*H*W][3C] rows, `table` [heads][(2ws-1)^2], dout
    [B*H*W][C] (and optionally the saved output `out`) -> dqkv [B*Hp*Wp][3C] over the PADDED,
    un-shifted grid (every row written, padding rows included) and dtable_part
    [window_partials_rows(B, H, W, ws)][heads * (2ws-1)^2] (column-sum it for d table)."""
    n, ldq = _rowmajor(qkv)
    nd, lddo = _rowmajor(dout)
    npad, lddq = _rowmajor(dqkv)
    hp, wp = -(-H // ws) * ws, -(-W // ws) * ws
    assert n == nd == B * H * W and qkv.shape[1] == 3 * C and dout.shape[1] == C
    assert npad == B * hp * wp and dqkv.shape[1] == 3 * C
    nrel = (2 * ws - 1) ** 2
    assert dtable_part.is_contiguous() and \
        dtable_part.numel() == window_partials_rows(B, H, W, ws) * heads * nrel
    ldo = 0
    if out is not None:
        no, ldo = _rowmajor(out)
        assert no == n and out.shape[1] == C
    flops = 12.0 * B * hp * wp * (ws * ws) * C
    _check(_launch("k_window_attn_bwd", flops, 40.0 * n * C,
                   lambda: lib().pn_window_attention_bwd_f32(
                       _ptr(qkv), ldq, _ptr(qkv_bias), _ptr(table), _ptr(dout), lddo, _ptr(out), ldo,
                       _ptr(dqkv), lddq, _ptr(dtable_part), B, H, W, C, heads, ws, shift, 32 ** -0.5,
                       _stream())), "pn_window_attention_bwd_f32")


def grad_norm_clip(g, out, scratch, pre=1.0, max_norm=0.0):
    """out[0] = ||pre * g||, out[1] = clip coefficient; g flat fp32, scratch >= 256 float64."""
    assert g.is_contiguous() and out.numel() >= 2 and scratch.numel() >= 256
    _check(lib().pn_grad_norm_clip_f32(_ptr(g), g.numel(), pre, max_norm, _ptr(out),
                                       _ptr(scratch, torch.float64), _stream()),
           "pn_grad_norm_clip_f32")


def adamw(p, g, m, v, seg_off, seg_lr, seg_wd, lr, beta1, beta2, eps, weight_decay, step,
          clip=None, pre=1.0, guard=None):
    """`guard`: an int32 device word (`loss_targets`' batch status); non-zero skips the whole
    update on the device (pn_adamw_guarded_f32)."""
    n = p.numel()
    assert all(t.is_contiguous() and t.numel() == n for t in (p, g, m, v))
    nseg = seg_lr.numel()
    assert seg_off.numel() == nseg + 1 and seg_wd.numel() == nseg
    if guard is not None:
        _check(lib().pn_adamw_guarded_f32(_ptr(p), _ptr(g), _ptr(m), _ptr(v), n,
                                          _ptr(seg_off, torch.int64), _ptr(seg_lr), _ptr(seg_wd),
                                          nseg, lr, beta1, beta2, eps, weight_decay, step,
                                          _ptr(clip), pre, _ptr(guard, torch.int32), _stream()),
               "pn_adamw_guarded_f32")
        return
    _check(lib().pn_adamw_f32(_ptr(p), _ptr(g), _ptr(m), _ptr(v), n, _ptr(seg_off, torch.int64),
                              _ptr(seg_lr), _ptr(seg_wd), nseg, lr, beta1, beta2, eps, weight_decay,
                              step, _ptr(clip), pre, _stream()), "pn_adamw_f32")


LSA_MAX_SIDE = 1024       # the larger side of a pn_lsa_f32 problem (csrc/assign.hip)


def lsa(cost, table, row_ind, col_ind, status, max_cells=0):
    """P = table.shape[0] assignment problems in one launch (`scipy.optimize.linear_sum_assignment`
    on the device, identical pairs).  cost: flat fp32; table [P][4] int64 on the device = (offset
    in cost, rows, cols, offset in row_ind / col_ind); row_ind / col_ind int32; status [P] int32
    (0 ok, 1 NaN / -inf entry, 2 infeasible, 3 descriptor out of range).  `max_cells`: the largest
    rows * cols, known from shapes on the host (sizes the LDS staging; 0: read from memory)."""
    assert table.dim() == 2 and table.shape[1] == 4 and table.is_contiguous()
    P = table.shape[0]
    assert cost.is_contiguous() and row_ind.numel() == col_ind.numel() and status.numel() >= P
    _check(lib().pn_lsa_f32(_ptr(cost), cost.numel(), _ptr(table, torch.int64), P, int(max_cells),
                            _ptr(row_ind, torch.int32), _ptr(col_ind, torch.int32),
                            row_ind.numel(), _ptr(status, torch.int32), _stream()), "pn_lsa_f32")


def loss_targets(lsa_table, row_ind, col_ind, lsa_status, tgt_table, gt, Q, R, importance, labels,
                 cum_samples, batch_status):
    """The loss targets of a batch from its 2B assignments (include/pairnet_hip.h): importance
    [B][Q][Q] fp32, labels [3][B*R] int64 (r_labels | sub_ids | obj_ids), cum_samples [C+1] fp32
    accumulated in place, batch_status [1] int32."""
    B = tgt_table.shape[0]
    assert lsa_table.shape == (2 * B, 4) and tgt_table.shape == (B, 4)
    assert lsa_table.is_contiguous() and tgt_table.is_contiguous() and gt.is_contiguous()
    assert importance.numel() == B * Q * Q and labels.numel() == 3 * B * R
    assert importance.is_contiguous() and labels.is_contiguous() and lsa_status.numel() >= 2 * B
    _check(lib().pn_loss_targets(_ptr(lsa_table, torch.int64), _ptr(row_ind, torch.int32),
                                 _ptr(col_ind, torch.int32), _ptr(lsa_status, torch.int32),
                                 _ptr(tgt_table, torch.int64), _ptr(gt, torch.int64), gt.numel(), B,
                                 Q, R, cum_samples.numel() - 1, _ptr(importance),
                                 _ptr(labels, torch.int64), _ptr(cum_samples),
                                 _ptr(batch_status, torch.int32), _stream()), "pn_loss_targets")


def bce_posw_mean(logits, target, out, loss_weight):
    _check(lib().pn_bce_posw_mean_f32(_ptr(logits), _ptr(target), _ptr(out), logits.numel(),
                                      loss_weight, _stream()), "pn_bce_posw_mean_f32")


# ---- the Mask2Former segmentation losses (csrc/seg_loss.hip; composed in seg_losses.py) ----------
SEG_SITE_ASSIGN, SEG_SITE_CANDIDATES, SEG_SITE_TAIL = 0, 1, 2   # site = 4 * layer + purpose


def uniform(out, seed, rank, step, site, site_stride=0):
    """out [nsites][n] (or [n]) <- Philox4x32-10 uniforms in [0, 1): element i of row s is word i % 4
    at counter (i / 4, rank, site + s * site_stride, step) under key `seed`, times 2^-24 after
    dropping its low 8 bits.  Nothing is uploaded; the same arguments give the same bits."""
    assert out.is_contiguous() and out.dim() in (1, 2)
    nsites = out.shape[0] if out.dim() == 2 else 1
    _check(lib().pn_uniform_f32(_ptr(out), out.shape[-1], nsites, site_stride, seed, rank, step,
                                site, _stream()), "pn_uniform_f32")


def seg_targets(table, row_ind, col_ind, lsa_status, gt_labels, L, B, Q, C, labels, matched, mcount,
                status):
    """include/pairnet_hip.h: labels [L][B*Q], matched [Mtot][4], mcount [L], status [1] from the
    L * B assignments (table [L*B][6] int64)."""
    assert table.shape == (L * B, 6) and table.is_contiguous() and labels.numel() == L * B * Q
    assert labels.is_contiguous() and matched.is_contiguous() and mcount.numel() >= L
    Mtot = matched.shape[0]
    assert matched.dim() == 2 and matched.shape[1] == 4 and row_ind.numel() == col_ind.numel()
    _check(lib().pn_seg_targets(_ptr(table, torch.int64), _ptr(row_ind, torch.int32),
                                _ptr(col_ind, torch.int32), _ptr(lsa_status, torch.int32),
                                lsa_status.numel(), _ptr(gt_labels, torch.int64), gt_labels.numel(),
                                row_ind.numel(), L, B, Q, C, Mtot, _ptr(labels, torch.int64),
                                _ptr(matched, torch.int64) if Mtot else None,
                                _ptr(mcount, torch.int32), _ptr(status, torch.int32), _stream()),
           "pn_seg_targets")


def uncertain_points(maps, matched, B, Q, cand, tail, k, keys, pts):
    """maps [nmaps][h][w] fp32, matched [M][4], cand [M][S][2], tail [M][Np-k][2] or None, keys
    [M][S] int32 (bit patterns of the sampled |logit|), pts [M][Np][2]."""
    nmaps, h, w = maps.shape
    M, S, _ = cand.shape
    Np = pts.shape[1]
    assert maps.is_contiguous() and matched.is_contiguous() and cand.is_contiguous() and \
        pts.is_contiguous() and keys.is_contiguous() and matched.shape == (M, 4)
    assert pts.shape == (M, Np, 2) and keys.shape == (M, S)
    assert tail is None or (tail.is_contiguous() and tail.shape == (M, Np - k, 2))
    _check(lib().pn_uncertain_points_f32(_ptr(maps), nmaps, _ptr(matched, torch.int64), M, B, Q, h, w,
                                         _ptr(cand), _ptr(tail), S, k, Np, _ptr(keys, torch.int32),
                                         _ptr(pts), _stream()), "pn_uncertain_points_f32")


def point_sample_rows(maps, idx, pts, out):
    """out[m][i] = map idx[m] of maps [nmaps][h][w] (fp32 or bool / uint8) at pts[m][i]."""
    nmaps, h, w = maps.shape
    M, Np, _ = pts.shape
    u8 = maps.dtype in (torch.bool, torch.uint8)
    assert maps.is_contiguous() and pts.is_contiguous() and out.is_contiguous()
    assert idx.numel() == M and out.shape == (M, Np)
    _check(lib().pn_point_sample_rows_f32(_ptr(maps, maps.dtype), int(u8), nmaps,
                                          _ptr(idx, torch.int64), _ptr(pts), _ptr(out), M, h, w, Np,
                                          _stream()), "pn_point_sample_rows_f32")


def mask_point_loss(x, t, matched, L, w_mask, w_dice, dice_eps, sums, out, coef=None,
                    num_total_masks=0.0):
    """x / t [M][Np], M = L * Ml; sums [M][4]; out [4L] = loss_mask | loss_dice | denominators; coef
    [M][Np] or None."""
    M, Np = x.shape
    assert M % L == 0 and t.shape == x.shape and x.is_contiguous() and t.is_contiguous()
    assert sums.numel() == 4 * M and out.numel() == 4 * L and matched.shape == (M, 4)
    assert coef is None or (coef.shape == x.shape and coef.is_contiguous())
    _check(lib().pn_mask_point_loss_f32(_ptr(x), _ptr(t), _ptr(matched, torch.int64), M, Np, L,
                                        M // L, w_mask, w_dice, dice_eps, num_total_masks,
                                        _ptr(sums), _ptr(out), _ptr(coef), _stream()),
           "pn_mask_point_loss_f32")


def point_scatter_scratch_ints(M, Np, h, w):
    return lib().pn_point_scatter_scratch_ints(M, Np, h, w)


def point_scatter_grad(coef, pts, grad, scratch):
    """grad [M][h][w] <- the transpose of the bilinear sample of coef [M][Np] at pts [M][Np][2]."""
    M, Np = coef.shape
    _, h, w = grad.shape
    assert coef.is_contiguous() and pts.is_contiguous() and grad.is_contiguous()
    assert pts.shape == (M, Np, 2) and grad.shape[0] == M
    assert scratch.numel() >= point_scatter_scratch_ints(M, Np, h, w)
    _check(lib().pn_point_scatter_grad_f32(_ptr(coef), _ptr(pts), _ptr(grad),
                                           _ptr(scratch, torch.int32), M, Np, h, w, _stream()),
           "pn_point_scatter_grad_f32")


def ce_avg(logits, target, class_weight, out, loss_weight):
    """logits [L][rows][C], target [L][rows] in [0, C), class_weight [C], out [L]."""
    L, rows, Cc = logits.shape
    assert logits.is_contiguous() and target.is_contiguous() and target.numel() == L * rows
    assert class_weight.numel() == Cc and out.numel() >= L
    _check(lib().pn_ce_avg_f32(_ptr(logits), _ptr(target, torch.int64), _ptr(class_weight),
                               _ptr(out), L, rows, Cc, loss_weight, _stream()), "pn_ce_avg_f32")


def ce_avg_grad(logits, target, class_weight, grad, loss_weight):
    L, rows, Cc = logits.shape
    assert logits.is_contiguous() and target.is_contiguous() and grad.is_contiguous()
    assert target.numel() == L * rows and class_weight.numel() == Cc and grad.shape == logits.shape
    _check(lib().pn_ce_avg_grad_f32(_ptr(logits), _ptr(target, torch.int64), _ptr(class_weight),
                                    _ptr(grad), L, rows, Cc, loss_weight, _stream()),
           "pn_ce_avg_grad_f32")


# ---- the sibling head's relation losses (csrc/rel_loss.hip; composed in baseline_losses.py) -------
REL_MAX_SIDE = 1024       # Q, R and the objects of one image (csrc/rel_loss.hip)
REL_STATUS_RANGE, REL_STATUS_TABLE, REL_STATUS_UNMATCHED, REL_STATUS_SEG = 4, 8, 16, 32


def rel_id_cost(rel, sub, obj, gt_rels, matched, tab, cost, w_s, w_o, w_r):
    """include/pairnet_hip.h: every image's [R, Gr_b] id match cost block of the flat `cost`, one
    launch.  rel [B, R, C1], sub / obj [B, R, Q] fp32; gt_rels [., 3], matched [Mtot, 4], tab [B, 8]
    int64."""
    B, R, C1 = rel.shape
    Q = sub.shape[2]
    assert sub.shape == (B, R, Q) and obj.shape == (B, R, Q) and tab.shape == (B, 8)
    assert all(t.is_contiguous() for t in (rel, sub, obj, gt_rels, matched, tab, cost))
    assert gt_rels.dim() == 2 and gt_rels.shape[1] == 3 and matched.dim() == 2 and matched.shape[1] == 4
    _check(lib().pn_rel_id_cost_f32(_ptr(rel), _ptr(sub), _ptr(obj), _ptr(gt_rels, torch.int64),
                                    gt_rels.shape[0], _ptr(matched, torch.int64), matched.shape[0],
                                    _ptr(tab, torch.int64), _ptr(cost), cost.numel(), B, R, Q, C1,
                                    w_s, w_o, w_r, _stream()), "pn_rel_id_cost_f32")


def rel_targets(tab, row_ind, col_ind, lsa_status, gt_rels, matched, R, Q, C1, r_labels, pos, status):
    """include/pairnet_hip.h: r_labels [B * R] int64, pos [P, 4] int32 and status [1] int32 from the B
    id assignments."""
    B = tab.shape[0]
    assert tab.shape == (B, 8) and tab.is_contiguous() and r_labels.numel() == B * R
    assert row_ind.numel() == col_ind.numel() == pos.shape[0] and pos.shape[1] == 4
    assert r_labels.is_contiguous() and pos.is_contiguous() and lsa_status.numel() >= B
    assert gt_rels.is_contiguous() and matched.is_contiguous()
    _check(lib().pn_rel_targets(_ptr(tab, torch.int64), _ptr(row_ind, torch.int32),
                                _ptr(col_ind, torch.int32), row_ind.numel(),
                                _ptr(lsa_status, torch.int32), _ptr(gt_rels, torch.int64),
                                gt_rels.shape[0], _ptr(matched, torch.int64), matched.shape[0], B, R,
                                Q, C1, _ptr(r_labels, torch.int64), _ptr(pos, torch.int32),
                                _ptr(status, torch.int32), _stream()), "pn_rel_targets")


def id_ce(sub, obj, matched, tab, pos, w_s, w_o, row_loss, out, g_sub=None, g_obj=None):
    """include/pairnet_hip.h: out [2] = loss_subject_match, loss_object_match; row_loss [P, 2];
    g_sub / g_obj [B, R, Q] (both or neither) are written in full."""
    B, R, Q = sub.shape
    assert obj.shape == sub.shape and sub.is_contiguous() and obj.is_contiguous()
    assert tab.shape == (B, 8) and tab.is_contiguous() and pos.is_contiguous() and pos.shape[1] == 4
    assert row_loss.numel() >= 2 * pos.shape[0] and out.numel() >= 2 and matched.is_contiguous()
    for g in (g_sub, g_obj):
        assert g is None or (g.shape == sub.shape and g.is_contiguous())
    _check(lib().pn_id_ce_f32(_ptr(sub), _ptr(obj), _ptr(matched, torch.int64), matched.shape[0],
                              _ptr(tab, torch.int64), _ptr(pos, torch.int32), pos.shape[0], B, R, Q,
                              w_s, w_o, _ptr(row_loss), _ptr(out), _ptr(g_sub), _ptr(g_obj),
                              _stream()), "pn_id_ce_f32")


# ---- the box head's object assignment cost (csrc/box_loss.hip; composed in bbox_losses.py) --------
def box_match_cost(cls, box, gt_labels, gt_bboxes, factor, tab, cost, max_cells, w_cls=2.0,
                   w_reg=5.0, w_iou=2.0, alpha=0.25, gamma=2.0, eps=1e-12, iou_eps=1e-6):
    """include/pairnet_hip.h: every image's [Q, G_b] box match cost block of the flat `cost`, one
    launch.  cls [B, Q, nc], box [B, Q, 4] (cxcywh, normalised), factor [B, 4] fp32; gt_labels [.]
    int64 and gt_bboxes [., 4] fp32 (xyxy, pixels) concatenated over the batch; tab [B, 4] int64 =
    (cost offset, G, label offset, box offset); `max_cells`: the largest Q * G_b."""
    B, Q, nc = cls.shape
    assert box.shape == (B, Q, 4) and factor.shape == (B, 4) and tab.shape == (B, 4)
    assert gt_bboxes.dim() == 2 and gt_bboxes.shape[1] == 4 and gt_labels.dim() == 1
    assert all(t.is_contiguous() for t in (cls, box, gt_labels, gt_bboxes, factor, tab, cost))
    _check(lib().pn_box_match_cost_f32(_ptr(cls), _ptr(box), _ptr(gt_labels, torch.int64),
                                       gt_labels.numel(), _ptr(gt_bboxes), gt_bboxes.shape[0],
                                       _ptr(factor), _ptr(tab, torch.int64), _ptr(cost),
                                       cost.numel(), int(max_cells), B, Q, nc, w_cls, w_reg, w_iou,
                                       alpha, gamma, eps, iou_eps, _stream()),
           "pn_box_match_cost_f32")


# ---- PSGTrHead2's triplet matching (csrc/tri_loss.hip; composed in psgtr2_losses.py) --------------
# sites of the counter-based draws (pn_uniform_f32), clear of seg_losses.py's 4 * layer + {0, 1, 2}
TRI_SITE_ASSIGN, TRI_SITE_SUB_CANDIDATES, TRI_SITE_SUB_TAIL = 1024, 1025, 1026
TRI_SITE_OBJ_CANDIDATES, TRI_SITE_OBJ_TAIL = 1027, 1028
TRI_STATUS_RANGE, TRI_STATUS_TABLE = 4, 8


def tri_match_cost_scratch(B, Q, SG, Np, device):
    """The scratch of `tri_match_cost` for B images, Q queries, SG objects in all, Np points."""
    f32 = lambda *s: torch.empty(*s, device=device, dtype=torch.float32)
    return dict(t=f32(SG, Np), tsum=f32(SG), stats=f32(3, B * Q, 2), pair=f32(2, SG, Q, 2),
                part=f32(4 * (SG + B) * Q * lib().pn_tri_pair_splits(B, Q, Np)))


def tri_match_cost(sub_cls, obj_cls, rel_cls, sub_maps, obj_maps, gt_masks, pts, gt_rels, gt_labels,
                   tab, weights, max_G, max_cells, cost, scratch=None):
    """include/pairnet_hip.h: every image's [Q, R_b] MaskHTriMatcher cost block of the flat `cost`,
    five launches.  sub_cls / obj_cls [B, Q, C1], rel_cls [B, Q, Cr1], sub_maps / obj_maps
    [B, Q, h, w] fp32; gt_masks [SG, hg, wg] uint8; pts [B, Np, 2]; gt_rels [., 3] and gt_labels [SG]
    int64; tab [B, 8] int64; weights: nine host floats (seven cost weights, two dice eps).
    -> the scratch dict(t [SG, Np], tsum [SG], stats [3, B * Q, 2], pair [2, SG, Q, 2], part: the
    pair sums of every point split, `tri_match_cost_scratch`)."""
    B, Q, C1 = sub_cls.shape
    Cr1 = rel_cls.shape[2]
    h, w = sub_maps.shape[2:]
    SG, hg, wg = gt_masks.shape
    Np = pts.shape[1]
    assert obj_cls.shape == (B, Q, C1) and rel_cls.shape[:2] == (B, Q) and tab.shape == (B, 8)
    assert sub_maps.shape == (B, Q, h, w) and obj_maps.shape == (B, Q, h, w)
    assert pts.shape == (B, Np, 2) and gt_masks.dtype == torch.uint8 and gt_labels.numel() == SG
    assert gt_rels.dim() == 2 and gt_rels.shape[1] == 3 and len(weights) == 9
    assert all(t.is_contiguous() for t in (sub_cls, obj_cls, rel_cls, sub_maps, obj_maps, gt_masks,
                                           pts, gt_rels, gt_labels, tab, cost))
    dev = sub_cls.device
    s = scratch or tri_match_cost_scratch(B, Q, SG, Np, dev)
    assert s["t"].shape == (SG, Np) and s["tsum"].numel() == SG and s["pair"].shape == (2, SG, Q, 2)
    assert s["stats"].shape == (3, B * Q, 2) and all(v.is_contiguous() for v in s.values())
    assert s["part"].numel() >= 4 * (SG + B) * Q * lib().pn_tri_pair_splits(B, Q, Np)
    wts = (C.c_float * 9)(*[float(v) for v in weights])
    _check(lib().pn_tri_match_cost_f32(
        _ptr(sub_cls), _ptr(obj_cls), _ptr(rel_cls), _ptr(sub_maps), _ptr(obj_maps),
        _ptr(gt_masks, torch.uint8), _ptr(pts), _ptr(gt_rels, torch.int64), gt_rels.shape[0],
        _ptr(gt_labels, torch.int64), SG, _ptr(tab, torch.int64), B, Q, C1, Cr1, h, w, hg, wg, Np,
        int(max_G), int(max_cells), C.cast(wts, C.c_void_p), _ptr(s["t"]), _ptr(s["tsum"]),
        _ptr(s["stats"]), _ptr(s["pair"]), _ptr(s["part"]), s["part"].numel(), _ptr(cost),
        cost.numel(), _stream()),
        "pn_tri_match_cost_f32")
    return s


def tri_targets(tab, row_ind, col_ind, lsa_status, gt_rels, gt_labels, Q, C, Cr, labels, matched,
                side_rows, rel_idx, mcount, status):
    """include/pairnet_hip.h: labels [3, B * Q], matched [M, 4], side_rows [2, M, 4], rel_idx [M]
    int64, mcount / status [1] int32 from the B assignments."""
    B = tab.shape[0]
    M = matched.shape[0]
    assert tab.shape == (B, 8) and tab.is_contiguous() and labels.shape == (3, B * Q)
    assert matched.shape == (M, 4) and side_rows.shape == (2, M, 4) and rel_idx.numel() == M
    assert row_ind.numel() == col_ind.numel() and lsa_status.numel() >= B
    assert all(t.is_contiguous() for t in (labels, matched, side_rows, rel_idx, gt_rels, gt_labels))
    _check(lib().pn_tri_targets(_ptr(tab, torch.int64), _ptr(row_ind, torch.int32),
                                _ptr(col_ind, torch.int32), row_ind.numel(),
                                _ptr(lsa_status, torch.int32), _ptr(gt_rels, torch.int64),
                                gt_rels.shape[0], _ptr(gt_labels, torch.int64), gt_labels.numel(), B,
                                Q, C, Cr, M, _ptr(labels, torch.int64), _ptr(matched, torch.int64),
                                _ptr(side_rows, torch.int64), _ptr(rel_idx, torch.int64),
                                _ptr(mcount, torch.int32), _ptr(status, torch.int32), _stream()),
           "pn_tri_targets")


# ---- the mask logits' backward (csrc/seg_grad.hip; composed in seg_grad.py) -----------------------
MASK_GRAD_MAX_ROWS = 65535
MASK_GRAD_KSLICE = 2048   # pn_mask_grad_kslice(): pixels per split-K slice, a function of P alone


def mask_grad_table(L, counts):
    """The host table of the two mask-gradient kernels, from shapes alone: `counts` = n_b =
    min(Q, G_b) per image, compact row m = l * sum(counts) + (rows of the images before b) + j.
    -> (int32 host tensor [img_off (B + 1) | order (M) | tiles (2 T)], T): `order` groups the rows
    by image (layers ascending), `tiles` are (image, offset into order) of the 32-row tiles of
    pn_mask_embed_grad_f32, none of which crosses an image."""
    L, counts = int(L), [int(c) for c in counts]
    if L <= 0 or not counts or min(counts) < 0:
        raise ValueError("L >= 1 layers and one non-negative row count per image")
    Ml = sum(counts)
    if L * Ml > MASK_GRAD_MAX_ROWS:
        raise ValueError("at most %d matched rows per call, got %d" % (MASK_GRAD_MAX_ROWS, L * Ml))
    img_off, order, tiles, m_off = [0], [], [], 0
    for b, n in enumerate(counts):
        order += [l * Ml + m_off + j for l in range(L) for j in range(n)]
        tiles += [v for s in range(img_off[-1], len(order), 32) for v in (b, s)]
        img_off.append(len(order))
        m_off += n
    return torch.tensor(img_off + order + tiles, dtype=torch.int32), len(tiles) // 2


def _mask_grad_args(G, mask_rows, table, B, T):
    if G.dim() != 2 or not G.is_contiguous():
        raise ValueError("G: contiguous [M, h * w], got %s" % (tuple(G.shape),))
    M, P = G.shape
    if M > MASK_GRAD_MAX_ROWS:
        raise ValueError("at most %d matched rows per call, got %d" % (MASK_GRAD_MAX_ROWS, M))
    if P <= 0:
        raise ValueError("G: no pixels")
    if mask_rows.dim() != 1 or mask_rows.shape[0] != M or not mask_rows.is_contiguous():
        raise ValueError("mask_rows: contiguous [%d], got %s" % (M, tuple(mask_rows.shape)))
    if table.dim() != 1 or not table.is_contiguous() or table.numel() != B + 1 + M + 2 * T:
        raise ValueError("table: %d + 1 + %d + 2 * %d int32 entries (mask_grad_table), got %d"
                         % (B, M, T, table.numel()))
    return M, P


def mask_embed_grad_scratch_floats(T, P):
    return int(lib().pn_mask_embed_grad_scratch_floats(int(T), int(P)))


def mask_embed_grad(G, MF, mask_rows, table, T, dme, scratch):
    """dme [M, 256] = G [M, P] x MF [B, P, 256] per image (include/pairnet_hip.h); `table`, `T`:
    `mask_grad_table` on the device; scratch: `mask_embed_grad_scratch_floats(T, P)` floats.
    Every row of dme is written (failed rows: zeros)."""
    if MF.dim() != 3 or MF.shape[2] != 256 or not MF.is_contiguous():
        raise ValueError("MF: contiguous [B, h * w, 256], got %s" % (tuple(MF.shape),))
    B = MF.shape[0]
    M, P = _mask_grad_args(G, mask_rows, table, B, T)
    if MF.shape[1] != P:
        raise ValueError("G has %d pixels per row, MF %d" % (P, MF.shape[1]))
    if tuple(dme.shape) != (M, 256) or not dme.is_contiguous():
        raise ValueError("dme: contiguous [%d, 256], got %s" % (M, tuple(dme.shape)))
    need = mask_embed_grad_scratch_floats(T, P)
    if M and (scratch is None or not scratch.is_contiguous() or scratch.numel() < need):
        raise ValueError("scratch: %d floats (mask_embed_grad_scratch_floats)" % need)
    _check(lib().pn_mask_embed_grad_f32(_ptr(G) if M else None, _ptr(MF),
                                        _ptr(mask_rows, torch.int64) if M else None,
                                        _ptr(table, torch.int32), table.numel(), M, B, T, P,
                                        _ptr(scratch) if M else None,
                                        scratch.numel() if M else 0, _ptr(dme) if M else None,
                                        _stream()), "pn_mask_embed_grad_f32")


def mask_feature_grad(G, me, mask_rows, table, T, dMF):
    """dMF [B, P, 256] = sum over the image's rows of G[m]^T x me[mask_rows[m]]
    (include/pairnet_hip.h); me [L * B * Q, 256].  Every element of dMF is written."""
    if dMF.dim() != 3 or dMF.shape[2] != 256 or not dMF.is_contiguous():
        raise ValueError("dMF: contiguous [B, h * w, 256], got %s" % (tuple(dMF.shape),))
    B = dMF.shape[0]
    if G.dim() == 2 and G.shape[0] == 0:            # no matched row at all: zeros
        G = G.new_empty(0, dMF.shape[1])
    M, P = _mask_grad_args(G, mask_rows, table, B, T)
    if dMF.shape[1] != P:
        raise ValueError("G has %d pixels per row, dMF %d" % (P, dMF.shape[1]))
    if me.dim() != 2 or me.shape[1] != 256 or not me.is_contiguous():
        raise ValueError("me: contiguous [L * B * Q, 256], got %s" % (tuple(me.shape),))
    _check(lib().pn_mask_feature_grad_f32(_ptr(G) if M else None, _ptr(me),
                                          _ptr(mask_rows, torch.int64) if M else None,
                                          _ptr(table, torch.int32), table.numel(), M, B, P,
                                          me.shape[0], _ptr(dMF), _stream()),
           "pn_mask_feature_grad_f32")


# ---- PSGTrHead2's three class heads, backward (csrc/tri_grad.hip; composed in seg_grad.py) --------
TRI_HEADS_MAX_ROWS, TRI_HEADS_MAX_C1, TRI_HEADS_MAX_CR1 = 4096, 256, 64


def tri_heads_bwd(dsub, dobj, drel, qn, Wsub, Wobj, Wrel, dqn, dWsub, dbsub, dWobj, dbobj, dWrel,
                  dbrel, add=False):
    """include/pairnet_hip.h, `pn_triplet_heads_bwd_f32`: dsub / dobj [N, C + 1], drel [N, Cr + 1] as
    the loss wrote them, qn [N, 256], the three weights in the reference layout -> dqn [N, 256]
    (`add`: onto what it holds) and the three dW [width, 256] / db [width], written whole.  Two
    launches, bitwise reproducible.  Shapes beyond the kernels' limits raise NotImplementedError."""
    if dsub.dim() != 2 or dobj.dim() != 2 or drel.dim() != 2 or qn.dim() != 2:
        raise ValueError("dsub / dobj [N, C + 1], drel [N, Cr + 1], qn [N, channels]")
    N, C1 = dsub.shape
    Cr1, ch = drel.shape[1], qn.shape[1]
    if ch != 256:
        raise NotImplementedError("256 channels per query row, got %d" % ch)
    if N > TRI_HEADS_MAX_ROWS:
        raise NotImplementedError("B * Q <= %d rows per call" % TRI_HEADS_MAX_ROWS)
    if C1 > TRI_HEADS_MAX_C1:
        raise NotImplementedError("C + 1 <= %d object classes per call" % TRI_HEADS_MAX_C1)
    if Cr1 > TRI_HEADS_MAX_CR1:
        raise NotImplementedError("Cr + 1 <= %d relation classes per call" % TRI_HEADS_MAX_CR1)
    if N <= 0 or C1 <= 0 or Cr1 <= 0:
        raise ValueError("no rows / classes")
    for name, t, shape in (("dsub", dsub, (N, C1)), ("dobj", dobj, (N, C1)), ("drel", drel, (N, Cr1)),
                           ("qn", qn, (N, 256)), ("dqn", dqn, (N, 256)),
                           ("Wsub", Wsub, (C1, 256)), ("Wobj", Wobj, (C1, 256)),
                           ("Wrel", Wrel, (Cr1, 256)), ("dWsub", dWsub, (C1, 256)),
                           ("dWobj", dWobj, (C1, 256)), ("dWrel", dWrel, (Cr1, 256)),
                           ("dbsub", dbsub, (C1,)), ("dbobj", dbobj, (C1,)), ("dbrel", dbrel, (Cr1,))):
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError("%s: contiguous %s, got %s" % (name, list(shape), tuple(t.shape)))
    _check(lib().pn_triplet_heads_bwd_f32(
        _ptr(dsub), _ptr(dobj), _ptr(drel), _ptr(qn), _ptr(Wsub), _ptr(Wobj), _ptr(Wrel), _ptr(dqn),
        _ptr(dWsub), _ptr(dbsub), _ptr(dWobj), _ptr(dbobj), _ptr(dWrel), _ptr(dbrel), N, 256, C1, Cr1,
        int(bool(add)), _stream()), "pn_triplet_heads_bwd_f32")


# ---- the training log on the device (csrc/train_log.hip) ----
LOG_MAX_TERMS = 32      # scalars per step one pn_train_log_row_f32 launch carries by value


def train_log_row(scalars, loss_mask, status, ring, row):
    """ONE launch: the step's T separate 0-dim float32 device scalars, the sum of those whose bit
    of `loss_mask` is set, the OR of the (up to two, int32) `status` words and the skipped flag
    -> row `row` of `ring` [rows][>= T + 3] (32-bit words, float32 tensor)."""
    T = len(scalars)
    if not 1 <= T <= LOG_MAX_TERMS:
        raise ValueError("train_log_row: %d scalars (1 .. %d)" % (T, LOG_MAX_TERMS))
    status = [s for s in status if s is not None]
    assert len(status) <= 2 and ring.dim() == 2 and ring.stride(1) == 1
    for v in scalars:
        assert v.numel() == 1, tuple(v.shape)
    ptrs = (_vp * T)(*[_ptr(v) for v in scalars])
    st = [_ptr(s, torch.int32) for s in status] + [None, None]
    _check(lib().pn_train_log_row_f32(ptrs, T, int(loss_mask) & 0xffffffff, st[0], st[1],
                                      _ptr(ring), ring.shape[0], ring.stride(0), int(row),
                                      _stream()), "pn_train_log_row_f32")


def train_log_window(ring, n, T, record):
    """One launch: the means of columns 0 .. T over rows [0, n) of `ring` in row order, the count
    of skipped rows, the OR of their status words and n -> `record` (>= T + 4 32-bit words)."""
    assert ring.dim() == 2 and ring.stride(1) == 1 and record.numel() >= T + 4
    assert record.is_contiguous()
    _check(lib().pn_train_log_window_f32(_ptr(ring), ring.shape[0], ring.stride(0), int(n), int(T),
                                         _ptr(record), _stream()), "pn_train_log_window_f32")


# ---- the plain Deformable-DETR detector's loss and box results (csrc/det_loss.hip; composed in
# det_losses.py / det_head.py) ----
DET_MAX_TERMS = 16      # terms of one pn_det_focal_f32 / pn_det_box_loss_f32 launch
DET_MAX_G = 1024        # ground-truth boxes of one pn_det_match_cost_f32 problem
DET_MAX_ROWS = 65536    # rows of one problem


def det_match_cost(cls, box, gt_labels, gt_bboxes, factor, tab, cost, max_cells, w_cls=2.0,
                   w_reg=5.0, w_iou=2.0, alpha=0.25, gamma=2.0, eps=1e-12, iou_eps=1e-6):
    """include/pairnet_hip.h: pn_box_match_cost_f32's cost for P problems of their own row counts,
    one launch.  cls [rows, nc] / box [rows, 4]: the problems' rows concatenated; gt_labels [.]
    int64, gt_bboxes [., 4] fp32 (xyxy, pixels); factor [P, 4]; tab [P, 6] int64 = (cost offset,
    rows, G, label offset, box offset, row offset); `max_cells`: the largest rows * G of the table
    (the caller's contract: the table is on the device, and cells past it are not written)."""
    rows, nc = cls.shape
    P = tab.shape[0]
    assert box.shape == (rows, 4) and factor.shape == (P, 4) and tab.shape == (P, 6)
    assert gt_bboxes.dim() == 2 and gt_bboxes.shape[1] == 4 and gt_labels.dim() == 1
    assert all(t.is_contiguous() for t in (cls, box, gt_labels, gt_bboxes, factor, tab, cost))
    _check(lib().pn_det_match_cost_f32(_ptr(cls), _ptr(box), rows, _ptr(gt_labels, torch.int64),
                                       gt_labels.numel(), _ptr(gt_bboxes), gt_bboxes.shape[0],
                                       _ptr(factor), _ptr(tab, torch.int64), _ptr(cost),
                                       cost.numel(), int(max_cells), P, nc, w_cls, w_reg, w_iou,
                                       alpha, gamma, eps, iou_eps, _stream()),
           "pn_det_match_cost_f32")


def det_focal_partials(rows, C, T):
    """Floats of pn_det_focal_f32's partial buffer (0: a shape the entry refuses)."""
    return int(lib().pn_det_focal_partials(int(rows), int(C), int(T)))


def det_focal(x, labels, term, avg, grad, partial, out, w_cls=2.0, alpha=0.25, gamma=2.0):
    """include/pairnet_hip.h: the focal term of every loss term in one launch over the concatenated
    rows.  x / grad [rows, C]; labels / term [rows] int32 (label C = background); avg [T] the
    terms' factors; out [T] = w_cls * sum / avg; grad = (w_cls / avg[term]) d loss / d x."""
    rows, C = x.shape
    T = avg.numel()
    assert grad.shape == x.shape and labels.shape == (rows,) and term.shape == (rows,)
    assert out.numel() == T
    assert all(t.is_contiguous() for t in (x, labels, term, avg, grad, partial, out))
    _check(lib().pn_det_focal_f32(_ptr(x), _ptr(labels, torch.int32), _ptr(term, torch.int32),
                                  _ptr(avg), _ptr(grad), _ptr(partial), partial.numel(), _ptr(out),
                                  rows, C, T, w_cls, alpha, gamma, _stream()), "pn_det_focal_f32")


def det_box_loss(box, gt_bboxes, factor, pairs, term_off, avg, grad, out, w_bbox=5.0, w_iou=2.0,
                 iou_eps=1e-6):
    """include/pairnet_hip.h: the L1 and GIoU terms over the matched pairs, one workgroup per term.
    box / grad [rows, 4] (grad zeroed by the caller); gt_bboxes [., 4]; factor [F, 4]; pairs [M, 4]
    int32 = (row, ground-truth box, factor row, term) grouped by term; term_off [T + 1] int32;
    out [T, 2] = (loss_bbox, loss_iou)."""
    rows, T, M = box.shape[0], avg.numel(), 0 if pairs is None else pairs.shape[0]
    assert box.shape == (rows, 4) == grad.shape and factor.dim() == 2 and factor.shape[1] == 4
    assert term_off.numel() == T + 1 and out.shape == (T, 2)
    assert M == 0 or (pairs.shape == (M, 4) and gt_bboxes.dim() == 2 and gt_bboxes.shape[1] == 4)
    ts = [t for t in (box, gt_bboxes, factor, pairs, term_off, avg, grad, out) if t is not None]
    assert all(t.is_contiguous() for t in ts)
    nb = 0 if gt_bboxes is None else gt_bboxes.shape[0]
    _check(lib().pn_det_box_loss_f32(_ptr(box), rows, _ptr(gt_bboxes) if nb else None, nb,
                                     _ptr(factor), factor.shape[0],
                                     _ptr(pairs, torch.int32) if M else None,
                                     _ptr(term_off, torch.int32), M, T, _ptr(avg), _ptr(grad),
                                     _ptr(out), w_bbox, w_iou, iou_eps, _stream()),
           "pn_det_box_loss_f32")


def det_results(cls, box, idx, meta, det, labels, rescale):
    """include/pairnet_hip.h: ranked flat indices idx [B, K] into cls [B, Q, C] -> det [B, K, 5]
    (clamped, optionally rescaled xyxy + sigmoid score) and labels [B, K] int64; meta [B, 6] =
    (img_h, img_w, scale_factor[0..3])."""
    B, Q, C = cls.shape
    K = idx.shape[1]
    assert box.shape == (B, Q, 4) and idx.shape == (B, K) and meta.shape == (B, 6)
    assert det.shape == (B, K, 5) and labels.shape == (B, K)
    assert all(t.is_contiguous() for t in (cls, box, idx, meta, det, labels))
    _check(lib().pn_det_results_f32(_ptr(cls), _ptr(box), _ptr(idx, torch.int64), _ptr(meta),
                                    _ptr(det), _ptr(labels, torch.int64), B, Q, C, K,
                                    1 if rescale else 0, _stream()), "pn_det_results_f32")
