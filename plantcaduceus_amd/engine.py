"""ctypes binding of libpcad.so (include/pcad.h) — PyTorch is plumbing only: device memory + streams.

The product path has NO CPU fallback: if the HIP library is missing, `load_library()` raises, and
`Engine.forward` refuses tensors that are not on a ROCm device.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import subprocess
from typing import Dict, Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PCAD_LIB") or os.path.join(_HERE, "libpcad.so")   # PCAD_LIB: developer A/B of two builds
CSRC = os.path.join(_HERE, "csrc")

PCAD_F32, PCAD_BF16 = 0, 1
_DT = {torch.float32: PCAD_F32, torch.bfloat16: PCAD_BF16}


class PcadConfig(C.Structure):
    _fields_ = [
        ("d_model", C.c_int32), ("n_layer", C.c_int32), ("d_state", C.c_int32), ("d_conv", C.c_int32),
        ("expand", C.c_int32), ("dt_rank", C.c_int32), ("vocab", C.c_int32), ("eps", C.c_float),
        ("dtype", C.c_int32), ("residual_in_fp32", C.c_int32), ("complement", C.c_int32 * 8),
    ]


class PcadKernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("launches", C.c_int64), ("total_ms", C.c_double)]


class PcadTensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("dtype", C.c_int32), ("ndim", C.c_int32),
                ("shape", C.c_int64 * 4)]


# name -> (restype, argtypes): every symbol include/pcad.h declares
SIGNATURES = {
    "pcad_version": (C.c_int, []),
    "pcad_last_error": (C.c_char_p, []),
    "pcad_build_hash": (C.c_char_p, []),
    "pcad_set_status_buffer": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pcad_create": (C.c_int, [C.POINTER(PcadConfig), C.POINTER(C.c_void_p)]),
    "pcad_destroy": (None, [C.c_void_p]),
    "pcad_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "pcad_weight_arena_bytes": (C.c_size_t, [C.c_void_p]),
    "pcad_bind_weights": (C.c_int, [C.c_void_p, C.POINTER(PcadTensor), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pcad_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "pcad_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pcad_forward_at": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_size_t, C.c_void_p]),
    "pcad_forward_all_hidden": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pcad_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "pcad_profile_read": (C.c_int, [C.c_void_p, C.POINTER(PcadKernelStat), C.c_int]),
    "pcad_add_rmsnorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                   C.c_float, C.c_int, C.c_int, C.c_void_p]),
    "pcad_causal_conv1d_silu": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pcad_causal_conv1d_silu_dir": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                              C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pcad_conv_xproj_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "pcad_conv_xproj_bidir": (C.c_int, [C.c_void_p] * 14 + [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pcad_selective_scan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_void_p]),
    "pcad_selective_scan_dtproj": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pcad_conv_xproj_split_scratch_bytes": (C.c_size_t, [C.c_int] * 6),
    "pcad_conv_xproj_bidir_engine": (C.c_int, [C.c_void_p] * 8 + [C.c_size_t] + [C.c_void_p] * 7 + [C.c_size_t] + [C.c_int] * 8 + [C.c_void_p]),
    "pcad_scan_segment_scratch_bytes": (C.c_size_t, [C.c_int] * 4),
    "pcad_selective_scan_engine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t] +
                                   [C.c_int] * 9 + [C.c_void_p]),
    "pcad_scan_pair_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "pcad_selective_scan_pair": (C.c_int, [C.c_void_p] * 15 + [C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t] +
                                 [C.c_int] * 7 + [C.c_void_p]),
    "pcad_gemm_nt": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                               C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pcad_gemm_nt_residual": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pcad_gemm_nt_split_scratch_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "pcad_gemm_nt_split": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                     C.c_void_p, C.c_size_t, C.c_void_p]),
    "pcad_gemm_nt_engine": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64] + [C.c_int] * 6 + [C.c_void_p]),
    "pcad_gemm_nt_xproj": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int,
                                     C.c_int64] + [C.c_int] * 5 + [C.c_void_p]),
    "pcad_gemm_nt_two": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64] +
                         [C.c_int] * 7 + [C.c_void_p]),
    "pcad_gemm_nt_residual_engine": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] +
                                     [C.c_int] * 5 + [C.c_void_p]),
    "pcad_gather_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int,
                                   C.c_void_p]),
    "pcad_final_head": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pcad_forward_pooled": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pcad_pooled_head_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "pcad_pooled_head": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                   C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "pcad_forward_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pcad_loss_head_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "pcad_loss_head": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                 C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pcad_forward_probs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_void_p,
                                     C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pcad_probs_head": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p,
                                  C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pcad_forward_layers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_void_p,
                                      C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pcad_layer_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_void_p,
                                  C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
}

# name -> (restype, argtypes): every symbol include/pcad_train.h declares (libpcad_train.so: the backward operators)
TRAIN_SIGNATURES = {
    "pcad_selective_scan_bwd_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "pcad_selective_scan_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 13 + [C.c_size_t] +
                                [C.c_int] * 5 + [C.c_void_p]),
}
TRAIN_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libpcad_train.so")

# name -> (restype, argtypes): every symbol include/pcad_bwd.h declares (libpcad_bwd.so: the conv, RMSNorm and loss head backward operators; the
# table, the header and the library's exports are held to each other, not to a closed list - later backward operators go here)
BWD_SIGNATURES = {
    "pcad_causal_conv1d_silu_bwd_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "pcad_causal_conv1d_silu_bwd": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 7 + [C.c_size_t] + [C.c_int] * 5 + [C.c_void_p]),
    "pcad_add_rmsnorm_bwd_scratch_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "pcad_add_rmsnorm_bwd": (C.c_int, [C.c_void_p] * 9 + [C.c_size_t, C.c_int64, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p]),
    "pcad_loss_head_bwd_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "pcad_loss_head_bwd": (C.c_int, [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 7 + [C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                     C.c_int, C.c_void_p]),
    "pcad_pooled_head_bwd_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "pcad_pooled_head_bwd": (C.c_int, [C.c_void_p] * 11 + [C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p]),
    # the score head on cached pooled vectors (plantcaduceus_amd.ops.pooled_logits / pooled_logits_bwd / pooled_logits_fn)
    "pcad_pooled_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pcad_pooled_logits_bwd": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_int, C.c_void_p]),
    # the optimizer step (plantcaduceus_amd.ops.OptimTable / adamw_step / zero_grads)
    "pcad_optim_plan": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "pcad_adamw_step_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "pcad_adamw_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_double] * 9 + [C.c_void_p]),
    "pcad_zero_grads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    # every gradient into one fp32 buffer for a collective (plantcaduceus_amd.ops.grads_flat_plan / grads_gather)
    "pcad_grads_flat_plan": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]),
    "pcad_grads_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    # the weight gradient of a linear layer into an fp32 main gradient (plantcaduceus_amd.ops.linear_wgrad / linear_fn)
    "pcad_linear_wgrad_slabs": (C.c_int64, [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "pcad_linear_wgrad_scratch_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "pcad_linear_wgrad": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p, C.c_size_t, C.c_void_p]),
    # the dropout-masked down-projection of a LoRA branch and its backward (plantcaduceus_amd.ops.lora_down / lora_down_bwd /
    # lora_dropout_linear_fn)
    "pcad_lora_dropout_mask": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_double, C.c_uint64, C.c_uint64, C.c_void_p]),
    "pcad_lora_down": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_uint64, C.c_uint64,
                                 C.c_int, C.c_void_p]),
    "pcad_lora_down_bwd_slabs": (C.c_int64, [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "pcad_lora_down_bwd_scratch_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "pcad_lora_down_bwd": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_int64, C.c_int, C.c_int, C.c_double, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]),
    # the selective scan's backward in segments (plantcaduceus_amd.ops.selective_scan_bwd(segments > 1))
    "pcad_selective_scan_bwd_seg_steps": (C.c_int, [C.c_int, C.c_int]),
    "pcad_selective_scan_bwd_seg_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "pcad_selective_scan_bwd_seg": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 13 + [C.c_size_t] +
                                    [C.c_int] * 6 + [C.c_void_p]),
    # the selective scan's training forward in segments (plantcaduceus_amd.ops.selective_scan_fwd_seg)
    "pcad_selective_scan_fwd_seg_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "pcad_selective_scan_fwd_seg": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 6 + [C.c_size_t] +
                                    [C.c_int] * 6 + [C.c_void_p]),
}
BWD_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libpcad_bwd.so")

# include/pcad.h pcad_pooling (pooling_strategy of CaduceusForSequenceClassification)
POOLING = {"mean": 0, "max": 1, "first": 2, "last": 3}
MAX_LABELS = 256
MAX_POSITIONS = 16      # include/pcad.h PCAD_MAX_POSITIONS



def check_layer_request(layers, n_layer: int, positions, positions_per_window, batch: Optional[int] = None):
    """The host-side argument rules of `Engine.forward_layers` / `hidden_states_at` (include/pcad.h pcad_forward_layers), raised as
    ValueError before anything is launched: layers None or strictly increasing indices inside [0, n_layer]; exactly one position
    form; 1..MAX_POSITIONS positions.  -> (levels list or None, P)."""
    lv = None
    if layers is not None:
        lv = [int(k) for k in layers]
        if not 1 <= len(lv) <= n_layer + 1:
            raise ValueError(f"layers must name 1..{n_layer + 1} levels, got {len(lv)}")
        if any(k < 0 or k > n_layer for k in lv):
            raise ValueError(f"layers must lie inside [0, {n_layer}] (0: the embedding output, {n_layer}: hidden_states[-1]), got {lv}")
        if any(b <= a for a, b in zip(lv, lv[1:])):
            raise ValueError(f"layers must be strictly increasing, got {lv}")
    if (positions is None) == (positions_per_window is None):
        raise ValueError("exactly one of positions and positions_per_window (all positions: output_hidden_states with "
                         "config.materialize_all_hidden_states)")
    if positions_per_window is not None:
        ppw = positions_per_window
        if (not torch.is_tensor(ppw) or ppw.is_floating_point() or ppw.dim() != 2 or (batch is not None and ppw.shape[0] != batch)
                or not 1 <= ppw.shape[1] <= MAX_POSITIONS):
            raise ValueError(f"positions_per_window must be an integer tensor [B, 1..{MAX_POSITIONS}]")
        return lv, int(ppw.shape[1])
    P = len(positions)
    if not 1 <= P <= MAX_POSITIONS:
        raise ValueError(f"positions must name 1..{MAX_POSITIONS} positions, got {P}")
    return lv, P


_lib = None

STATUS_BAD_TOKEN, STATUS_BAD_POSITION, STATUS_BAD_LABEL = 1, 2, 4       # include/pcad.h pcad_status_bits


def source_hash() -> str:
    """sha1 over csrc/*.hip, *.hpp (csrc/source_hash.py: the value the Makefile bakes into libpcad.so as pcad_build_hash)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_pcad_source_hash", os.path.join(CSRC, "source_hash.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.source_hash(CSRC)


def build_library(force: bool = False) -> str:
    """Compile the HIP sources in-tree (`hipcc --offload-arch=gfx950`, cross-compiles without a GPU)."""
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, capture_output=True)
    r = subprocess.run(["make", "-C", CSRC, "-j", "6"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libpcad.so failed:\n" + r.stdout[-4000:] + "\n" + r.stderr[-4000:])
    return LIB_PATH


def _bind_library(path: str, signatures, missing_message: str):
    """CDLL(path) with restype / argtypes set for every symbol of `signatures`; a missing file raises RuntimeError(missing_message),
    a missing symbol AttributeError"""
    if not os.path.exists(path):
        raise RuntimeError(missing_message)
    lib = C.CDLL(path)
    for name, (res, args) in signatures.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library():
    """Load libpcad.so; fails loudly if it is missing (no CPU fallback on the product path)."""
    global _lib
    if _lib is not None:
        return _lib
    lib = _bind_library(LIB_PATH, SIGNATURES,
                        f"{LIB_PATH} not found: the MI355X HIP extension is not built. Run "
                        "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C plantcaduceus_amd/csrc`). "
                        "There is deliberately no CPU fallback.")
    # a binary that was not built from the sources beside it would silently run (and be benchmarked as) other kernels
    if os.path.exists(os.path.join(CSRC, "source_hash.py")) and os.environ.get("PCAD_ALLOW_STALE") != "1":
        built, have = lib.pcad_build_hash().decode(), source_hash()
        if built != have:
            raise RuntimeError(
                f"{LIB_PATH} was built from other kernel sources (pcad_build_hash {built}, sources {have}): rebuild it with "
                "`make -C plantcaduceus_amd/csrc` / `__graft_entry__.build()` (PCAD_ALLOW_STALE=1 overrides, for A/B of old builds)")
    _lib = lib
    return lib


_backward_libs = {}      # path -> the loaded library, once per process


def _load_beside(path: str, signatures):
    """a backward library beside libpcad.so, which it links and which is loaded first"""
    if path not in _backward_libs:
        load_library()
        _backward_libs[path] = _bind_library(path, signatures, f"{path} not found: build it with `make -C plantcaduceus_amd/csrc` / "
                                                                "`__graft_entry__.build()`")
    return _backward_libs[path]


def load_train_library():
    """Load libpcad_train.so (include/pcad_train.h) beside libpcad.so, which it links and which is loaded first; fails loudly if it
    is missing - a missing backward kernel is an error, there is no fallback to torch."""
    return _load_beside(TRAIN_LIB_PATH, TRAIN_SIGNATURES)


def load_bwd_library():
    """Load libpcad_bwd.so (include/pcad_bwd.h), likewise."""
    return _load_beside(BWD_LIB_PATH, BWD_SIGNATURES)


def _check(code: int, what: str):
    if code != 0:
        msg = load_library().pcad_last_error()
        raise RuntimeError(f"{what} failed ({code}): {msg.decode() if msg else ''}")


def _stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def _require_gpu(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on a ROCm device (got {t.device}); the MI355X engine has no CPU path")


class Engine:
    """One handle = one model on one GPU.  Owns (as torch tensors) the weight arena and workspace."""

    def __init__(self, config, state_dict: Dict[str, torch.Tensor], dtype: torch.dtype, device: torch.device):
        if dtype not in _DT:
            raise ValueError(f"unsupported dtype {dtype}: the engine computes in bf16 or fp32")
        config.check_supported()
        self.lib = load_library()
        self.config = config
        self.dtype = dtype
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the MI355X engine needs a ROCm device ('cuda:N'); there is no CPU path")
        cfg = PcadConfig(
            d_model=config.d_model, n_layer=config.n_layer, d_state=config.d_state, d_conv=config.d_conv,
            expand=config.expand, dt_rank=config.dt_rank, vocab=config.padded_vocab_size, eps=config.norm_epsilon,
            dtype=_DT[dtype], residual_in_fp32=int(bool(config.residual_in_fp32)),
            complement=(C.c_int32 * 8)(*config.complement_list()[:8]))
        self._h = C.c_void_p()
        _check(self.lib.pcad_create(C.byref(cfg), C.byref(self._h)), "pcad_create")
        self._ws: Optional[torch.Tensor] = None
        if not getattr(config, "bidirectional_weight_tie", True):
            self.set_option("untied_directions", 1)      # mamba_rev has its own in_proj / out_proj: bound beside mamba_fwd's
        for key, val in (getattr(config, "engine_options", None) or {}).items():
            self.set_option(key, int(val))
        with torch.cuda.device(self.device):
            nbytes = self.lib.pcad_weight_arena_bytes(self._h)
            self._arena = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
            self._bind(state_dict)
            # input-validation flags: a device word the kernels OR bits into + a pinned host mirror filled by an async copy
            with torch.inference_mode(False):      # normal tensors: they are updated in place from inside AND outside inference mode
                self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
                self._status_host = torch.zeros(1, dtype=torch.int32).pin_memory()
            self._status_event = torch.cuda.Event()
            self._status_event.record()
            _check(self.lib.pcad_set_status_buffer(self._h, self._status.data_ptr()), "pcad_set_status_buffer")

    def _aligned(self, t: torch.Tensor) -> int:
        return (t.data_ptr() + 255) // 256 * 256

    def _bind(self, sd: Dict[str, torch.Tensor]):
        keep = []
        arr = (PcadTensor * len(sd))()
        n = 0
        for name, t in sd.items():
            if not torch.is_tensor(t) or not t.is_floating_point():
                continue
            tt = t.detach()
            if tt.dtype not in _DT:
                tt = tt.float()
            tt = tt.to(self.device).contiguous()
            keep.append(tt)
            shape = list(tt.shape)[:4] + [1] * (4 - min(4, tt.dim()))
            if tt.dim() > 4:
                raise ValueError(name)
            arr[n] = PcadTensor(name.encode(), tt.data_ptr(), _DT[tt.dtype], min(4, tt.dim()), (C.c_int64 * 4)(*shape))
            n += 1
        base = self._aligned(self._arena)
        _check(self.lib.pcad_bind_weights(self._h, arr, n, base, self._arena.numel() - (base - self._arena.data_ptr()),
                                          _stream_ptr()), "pcad_bind_weights")
        torch.cuda.current_stream().synchronize()   # source tensors in `keep` may be freed after this
        del keep

    def _workspace(self, B: int, L: int):
        need = self.lib.pcad_workspace_bytes(self._h, B, L)
        if self._ws is None or self._ws.numel() < need + 256:
            self._ws = None
            self._ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        base = self._aligned(self._ws)
        return base, self._ws.numel() - (base - self._ws.data_ptr())

    def _check_ids(self, input_ids: torch.Tensor):
        """The checks every forward makes on its ids [B, L] -> (B, L).  Nothing is enqueued here."""
        _require_gpu(input_ids, "input_ids")
        if input_ids.dim() != 2:
            raise ValueError(f"input_ids must be [B, L], got {tuple(input_ids.shape)}")
        if input_ids.device != self.device:
            raise RuntimeError(f"input_ids on {input_ids.device}, engine on {self.device}")
        return input_ids.shape[0], input_ids.shape[1]

    def _ids(self, input_ids: torch.Tensor) -> torch.Tensor:
        """What follows a forward's argument checks: an earlier forward's pending IndexError, then the int32 copy of the ids."""
        self._poll_status()
        return input_ids.to(torch.int32).contiguous()

    @contextlib.contextmanager
    def _call(self, B: int, L: int):
        """Around one pcad_forward* call -> (workspace, bytes); then the status word follows it on the stream into pinned host memory."""
        ws = self._workspace(B, L)
        try:
            yield ws
        finally:
            self._status_host.copy_(self._status, non_blocking=True)
            self._status_event.record()

    @staticmethod
    def _narrow_positions(ppw: torch.Tensor) -> torch.Tensor:
        """int64 positions are clamped before they are narrowed to int32, so that a huge value cannot alias a valid one."""
        return ppw.clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32).contiguous()

    def forward(self, input_ids: torch.Tensor, positions=None,
                want_hidden: bool = False, want_logits: bool = True, all_hidden: bool = False):
        """ids [B, L] (any int dtype, on this device) -> (logits fp32 [B,Q,8] | None, hidden [B,Q,2D] | None[, all]).
        positions: None (all L), a short list shared by every window, or an integer tensor [B] on this device
        (one position per window, Q = 1).

        Nothing here synchronises with the device.  Token ids outside the vocabulary and per-window positions outside the
        window - for which the reference raises an index error - are detected by the forward's last kernel and reported
        asynchronously: `check_status()` (which the host loops of this package call where they read results back) raises
        IndexError, and so does the next `forward` call once the flag of an earlier one has arrived."""
        B, L = self._check_ids(input_ids)
        ids = self._ids(input_ids)
        D = self.config.d_model
        per_seq = None
        if torch.is_tensor(positions):
            if positions.dim() != 1 or positions.shape[0] != B or positions.device != self.device:
                raise ValueError("per-window positions must be an integer tensor [B] on the engine's device")
            per_seq = positions.to(torch.int32).contiguous()
            positions = None
        P = 0 if positions is None else len(positions)
        Q = 1 if per_seq is not None else (P if P else L)
        with torch.cuda.device(self.device):
            logits = torch.empty((B, Q, 8), dtype=torch.float32, device=self.device) if want_logits else None
            hidden = torch.empty((B, Q, 2 * D), dtype=self.dtype, device=self.device) if want_hidden else None
            if B == 0:
                return (logits, hidden, None) if all_hidden else (logits, hidden)
            lp = logits.data_ptr() if logits is not None else None
            hp = hidden.data_ptr() if hidden is not None else None
            with self._call(B, L) as (ws, ws_bytes):
                if all_hidden:
                    if positions is not None or per_seq is not None:
                        raise ValueError("all_hidden requires positions=None")
                    allh = torch.empty((self.config.n_layer, B, L, 2 * D), dtype=self.dtype, device=self.device)
                    _check(self.lib.pcad_forward_all_hidden(self._h, ids.data_ptr(), B, L, allh.data_ptr(), hp, lp, ws,
                                                            ws_bytes, _stream_ptr()), "pcad_forward_all_hidden")
                    return logits, hidden, allh
                if per_seq is not None:
                    _check(self.lib.pcad_forward_at(self._h, ids.data_ptr(), B, L, per_seq.data_ptr(), hp, lp, ws, ws_bytes,
                                                    _stream_ptr()), "pcad_forward_at")
                    return logits, hidden
                pos_arr = (C.c_int32 * P)(*[int(p) for p in positions]) if P else None
                _check(self.lib.pcad_forward(self._h, ids.data_ptr(), B, L, pos_arr, P, hp, lp, ws, ws_bytes,
                                             _stream_ptr()), "pcad_forward")
        return logits, hidden

    def forward_pooled(self, input_ids: torch.Tensor, pooling: str, score_w: torch.Tensor, want_pooled: bool = False):
        """Sequence classification (`pcad_forward_pooled`): ids [B, L] on this device -> logits fp32 [B, NL] (and, with
        want_pooled, the pooled vectors fp32 [B, 2, D]: [:, 0] the window's strand, [:, 1] its reverse complement's).
        pooling: "mean" / "max" / "first" / "last"; score_w: the `score` Linear's weight [NL, D] (any float dtype, any device),
        rounded to the model dtype here as the reference's `nn.Linear` in that dtype holds it.  Chunking, workspace and
        asynchronous input validation are those of `forward`."""
        B, L = self._check_ids(input_ids)
        if pooling not in POOLING:
            raise ValueError(f"pooling must be one of {sorted(POOLING)}, got {pooling!r}")
        D = self.config.d_model
        if score_w.dim() != 2 or score_w.shape[1] != D or not 1 <= score_w.shape[0] <= MAX_LABELS:
            raise ValueError(f"score weight must be [num_labels (1..{MAX_LABELS}), {D}], got {tuple(score_w.shape)}")
        ids = self._ids(input_ids)
        NL = int(score_w.shape[0])
        with torch.cuda.device(self.device):
            w = score_w.detach().to(self.device).to(self.dtype).float().contiguous()
            logits = torch.empty((B, NL), dtype=torch.float32, device=self.device)
            pooled = torch.empty((B, 2, D), dtype=torch.float32, device=self.device) if want_pooled else None
            if B == 0:
                return (logits, pooled) if want_pooled else logits
            with self._call(B, L) as (ws, ws_bytes):
                _check(self.lib.pcad_forward_pooled(self._h, ids.data_ptr(), B, L, POOLING[pooling], w.data_ptr(), NL,
                                                    pooled.data_ptr() if pooled is not None else None, logits.data_ptr(),
                                                    ws, ws_bytes, _stream_ptr()), "pcad_forward_pooled")
        return (logits, pooled) if want_pooled else logits

    def forward_loss(self, input_ids: torch.Tensor, labels: torch.Tensor, loss_weights: Optional[torch.Tensor] = None,
                     ignore_index: int = -100, want_nll: bool = False, want_logits: bool = False):
        """Masked-LM loss (`pcad_forward_loss`): ids / labels [B, L] (any int dtype) and loss_weights [B, L] (any float dtype) or
        None, on this device -> (sums fp32 [B, 4], nll fp32 [B, L] | None, logits fp32 [B, L, 8] | None).  sums[b] = (sum w nll,
        sum w, labelled positions, labelled positions whose arg-max logit is the label) of window b; a label equal to
        ignore_index or negative is ignored, any other label outside the vocabulary is reported like a bad token id
        (`check_status`).  Chunking, workspace and asynchronous input validation are those of `forward`."""
        B, L = self._check_ids(input_ids)
        if not torch.is_tensor(labels) or tuple(labels.shape) != tuple(input_ids.shape) or labels.is_floating_point():
            raise ValueError(f"labels must be an integer tensor of input_ids' shape {tuple(input_ids.shape)}")
        if loss_weights is not None and (not torch.is_tensor(loss_weights) or tuple(loss_weights.shape) != tuple(input_ids.shape)):
            raise ValueError(f"loss_weights must be a tensor of input_ids' shape {tuple(input_ids.shape)}")
        if not -2 ** 31 <= int(ignore_index) < 2 ** 31:
            raise ValueError("ignore_index must fit in 32 bits")
        ids = self._ids(input_ids)
        with torch.cuda.device(self.device):
            # int64 labels are clamped before they are narrowed, so that a huge value cannot alias a valid one
            lab = labels.to(self.device).clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32).contiguous()
            w = loss_weights.to(self.device).to(torch.float32).contiguous() if loss_weights is not None else None
            sums = torch.empty((B, 4), dtype=torch.float32, device=self.device)
            nll = torch.empty((B, L), dtype=torch.float32, device=self.device) if want_nll else None
            logits = torch.empty((B, L, 8), dtype=torch.float32, device=self.device) if want_logits else None
            if B == 0:
                return sums, nll, logits
            with self._call(B, L) as (ws, ws_bytes):
                _check(self.lib.pcad_forward_loss(self._h, ids.data_ptr(), lab.data_ptr(), w.data_ptr() if w is not None else None,
                                                  int(ignore_index), B, L, sums.data_ptr(), nll.data_ptr() if nll is not None else None,
                                                  logits.data_ptr() if logits is not None else None, ws, ws_bytes, _stream_ptr()),
                       "pcad_forward_loss")
        return sums, nll, logits

    def forward_probs(self, input_ids: torch.Tensor, cols, positions=None, positions_per_window: Optional[torch.Tensor] = None,
                      want_logits: bool = False):
        """Nucleotide probabilities (`pcad_forward_probs`): ids [B, L] on this device -> probs fp32 [B, Q, 4] (and, with
        want_logits, the logits fp32 [B, Q, 8] they were formed from): the softmax over the four vocabulary columns `cols` of the
        LM head's logits, taken on the device.  positions: None (all L) or a short list shared by every window;
        positions_per_window: an integer tensor [B, P] (1 <= P <= 16) on this device, window b's own positions - a value outside
        [0, L) is clamped and reported like a bad token id (`check_status`).  At most one of the two.  Chunking, workspace and
        asynchronous input validation are those of `forward`."""
        B, L = self._check_ids(input_ids)
        cols = [int(c) for c in cols]
        if len(cols) != 4:
            raise ValueError(f"cols must name four vocabulary columns, got {cols}")
        if positions is not None and positions_per_window is not None:
            raise ValueError("positions and positions_per_window are exclusive")
        ids = self._ids(input_ids)
        ppw = positions_per_window
        if ppw is not None:
            if (not torch.is_tensor(ppw) or ppw.is_floating_point() or ppw.dim() != 2 or ppw.shape[0] != B
                    or not 1 <= ppw.shape[1] <= MAX_POSITIONS or ppw.device != self.device):
                raise ValueError(f"positions_per_window must be an integer tensor [B, 1..{MAX_POSITIONS}] on the engine's device")
            ppw = self._narrow_positions(ppw)
            P = int(ppw.shape[1])
        else:
            P = 0 if positions is None else len(positions)
        Q = P if P else L
        with torch.cuda.device(self.device):
            probs = torch.empty((B, Q, 4), dtype=torch.float32, device=self.device)
            logits = torch.empty((B, Q, 8), dtype=torch.float32, device=self.device) if want_logits else None
            if B == 0:
                return (probs, logits) if want_logits else probs
            pos_arr = (C.c_int32 * P)(*[int(p) for p in positions]) if (P and ppw is None) else None
            with self._call(B, L) as (ws, ws_bytes):
                _check(self.lib.pcad_forward_probs(self._h, ids.data_ptr(), B, L, pos_arr, P, ppw.data_ptr() if ppw is not None else None,
                                                   (C.c_int32 * 4)(*cols), probs.data_ptr(),
                                                   logits.data_ptr() if logits is not None else None, ws, ws_bytes, _stream_ptr()),
                       "pcad_forward_probs")
        return (probs, logits) if want_logits else probs

    def forward_layers(self, input_ids: torch.Tensor, layers=None, positions=None, positions_per_window: Optional[torch.Tensor] = None,
                       average: bool = False):
        """Hidden states of chosen levels at the evaluated positions (`pcad_forward_layers`): ids [B, L] on this device ->
        [NL, B, P, 2D] in the model dtype, or - average - the reverse-complement-averaged fp32 embedding [NL, B, P, D].
        layers: None (all n_layer + 1 levels of the reference's `hidden_states` tuple) or strictly increasing indices into it (0: the
        embedding output, n_layer: hidden_states[-1]).  Exactly one of positions (1..16 positions shared by every window) and
        positions_per_window (an integer tensor [B, 1..16] on this device; a value outside [0, L) is clamped and reported like a bad
        token id, `check_status`).  Only the last level asked for: `forward`'s own walk; any level below it: the unfolded walk of
        `forward(all_hidden=True)`, whose levels the rows are bit-equal to, run only as deep as the highest level asked for.
        Chunking, workspace and asynchronous input validation are those of `forward`."""
        B, L = self._check_ids(input_ids)
        lv, P = check_layer_request(layers, self.config.n_layer, positions, positions_per_window, B)
        ids = self._ids(input_ids)
        ppw = positions_per_window
        if ppw is not None:
            if ppw.device != self.device:
                raise ValueError("positions_per_window must be on the engine's device")
            ppw = self._narrow_positions(ppw)
        positions = None if positions is None else [int(p) for p in positions]
        D = self.config.d_model
        NL = len(lv) if lv is not None else self.config.n_layer + 1
        with torch.cuda.device(self.device):
            out = torch.empty((NL, B, P, D if average else 2 * D), dtype=torch.float32 if average else self.dtype, device=self.device)
            if B == 0:
                return out
            pos_arr = (C.c_int32 * P)(*positions) if ppw is None else None
            lay_arr = (C.c_int32 * NL)(*lv) if lv is not None else None
            with self._call(B, L) as (ws, ws_bytes):
                _check(self.lib.pcad_forward_layers(self._h, ids.data_ptr(), B, L, pos_arr, P, ppw.data_ptr() if ppw is not None else None,
                                                    lay_arr, NL if lv is not None else 0, int(bool(average)), out.data_ptr(), ws, ws_bytes,
                                                    _stream_ptr()), "pcad_forward_layers")
        return out

    # -- asynchronous input validation (include/pcad.h pcad_set_status_buffer) ----------------------------------------
    def _raise_status(self, bits: int):
        self._status.zero_()
        self._status_host.zero_()
        V = int(self.config.padded_vocab_size)
        what = []
        if bits & STATUS_BAD_TOKEN:
            what.append(f"input_ids contain token ids outside [0, {V}): check the tokenizer's vocabulary against the model")
        if bits & STATUS_BAD_POSITION:
            what.append("a per-window position is outside [0, L)")
        if bits & STATUS_BAD_LABEL:
            what.append(f"labels contain values that are neither ignored (ignore_index or negative) nor inside [0, {V})")
        raise IndexError("; ".join(what) + " (detected on the device; results of that forward are invalid)")

    def _poll_status(self):
        """Non-blocking: raises if the status word of an EARLIER forward has already arrived and is set."""
        if self._status_event.query() and int(self._status_host[0]) != 0:
            self._raise_status(int(self._status_host[0]))

    def status_bits(self) -> int:
        """Blocking, non-raising: waits for the forwards enqueued so far and returns their accumulated status bits (0 = clean).
        Distributed host loops reduce this over the ranks first, so that every rank raises together (zero_shot.check_model_inputs)."""
        self._status_event.synchronize()
        return int(self._status_host[0])

    def check_status(self, bits: Optional[int] = None):
        """Blocking: waits for the forwards enqueued so far and raises IndexError if any of them saw an invalid token id or
        position (the reference's nn.Embedding / indexing errors).  Host loops call this where they read results back.
        bits: status bits already collected (e.g. OR-ed over the ranks of a process group) instead of this engine's own."""
        if bits is None:
            bits = self.status_bits()
        if bits:
            self._raise_status(bits)

    def set_option(self, key: str, value: int):
        """`pcad_set_option` (include/pcad.h): "chunk_seqs" (windows per pass through the stack), "gate_each" (reference-order
        SiLU gate), "norm_fold" (add + RMSNorm folded into out_proj's epilogue / in_proj), "reference_order" (0 / 1 / 2: one switch for
        the reference's rounding points), "f32_gemm_split" (fp32 model: split-bf16 in_proj / out_proj), "untied_directions" (mamba_rev's
        own in_proj / out_proj: merged LoRA deltas, bidirectional_weight_tie=False), "scan_segments" (segmented scan of long strands),
        "last_layer_shortcut", "poison_workspace" (debug).  "norm_fold" 1 on an fp32 model, "f32_gemm_split" and "untied_directions"
        need weights packed at bind time: pass them as `config.engine_options` (applied before binding)."""
        _check(self.lib.pcad_set_option(self._h, key.encode(), int(value)), "pcad_set_option")
        self._ws = None

    def release_workspace(self):
        """Free the workspace slab (it is re-allocated by the next forward): for a process that keeps several models resident
        and runs them in turn.  `set_option("workspace_limit_mb", N)` bounds what a forward allocates in the first place."""
        self._ws = None

    def profile(self, on):
        """False/0: off; True/1: HIP events around every launch; N > 1: around every N-th launch of each kernel class."""
        _check(self.lib.pcad_profile_enable(self._h, int(on)), "pcad_profile_enable")

    def profile_read(self):
        """-> {kernel class: (launches, total_ms)} since the last read (waits for the events)."""
        arr = (PcadKernelStat * 16)()
        n = self.lib.pcad_profile_read(self._h, arr, 16)
        if n < 0:
            _check(n, "pcad_profile_read")
        return {arr[i].name.decode(): (int(arr[i].launches), float(arr[i].total_ms)) for i in range(n)}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.pcad_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
