"""ctypes binding of liblanefit_hip.so (the C ABI in include/lanefit.h).

The library is the product: there is no eager / CPU fallback.  If it is missing, or a call
is made without a GPU tensor, this module raises -- loudly -- instead of computing anything.
"""
import ctypes
import os
from ctypes import c_char_p, c_double, c_int, c_long, c_size_t, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblanefit_hip.so")
_lib = None


class LaneFitLibraryError(RuntimeError):
    pass


def _declare(lib):
    P, I, L, D = c_void_p, c_int, c_long, c_double
    sig = {
        "lf_abi_version": (c_int, []),
        "lf_last_error": (c_char_p, []),
        "lf_wls_workspace_bytes": (c_size_t, [I, I, I]),
        "lf_wls_fwd": (I, [P, P, L, I, I, I, I, I, I, D, D, I, I, P, P, P, P, P, P]),
        "lf_wls_bwd": (I, [P, P, L, I, I, I, I, I, I, D, I, P, P, P, P, P]),
        "lf_gels_workspace_bytes": (c_size_t, [I, I]),
        "lf_gels_fwd": (I, [P, P, I, L, I, P, P, P, P, P]),
        "lf_gels_bwd": (I, [P, P, P, P, P, I, L, I, P, P, P]),
        "lf_area_loss": (I, [P, L, P, I, I, I, I, P, P, P]),
        "lf_mse_loss": (I, [P, P, L, I, P, P, P]),
        "lf_backproj_loss": (I, [P, L, P, P, P, P, P, I, I, I, P, P, P, P]),
        "lf_ce2d_fwd": (I, [P, P, P, I, I, I, I, P, P, P]),
        "lf_ce2d_bwd": (I, [P, P, P, I, I, I, I, P, P, P, P]),
        "lf_erfnet_plan_create": (P, [I, I, I, I, I, I]),
        "lf_erfnet_plan_destroy": (None, [P]),
        "lf_erfnet_workspace_bytes": (c_size_t, [P]),
        "lf_erfnet_workspace_bytes_for": (c_size_t, [P, I]),
        "lf_erfnet_activation_floats": (L, [P]),
        "lf_erfnet_num_params": (I, [P]),
        "lf_erfnet_num_bn": (I, [P]),
        "lf_erfnet_num_dropout": (I, [P]),
        "lf_erfnet_dropmask_floats": (L, [P]),
        "lf_erfnet_dropmask_offset": (L, [P, I]),
        "lf_erfnet_dropmask_channels": (I, [P, I]),
        "lf_erfnet_encoder_offset": (L, [P]),
        "lf_erfnet_activation_offset": (L, [P, I, I]),
        "lf_erfnet_bn_vector_offset": (L, [P, I, I, I]),
        "lf_erfnet_forward": (I, [P, P, P, P, P, P, I, I, P, P, c_size_t, P]),
        "lf_erfnet_backward": (I, [P, P, P, P, P, P, P, I, I, P, c_size_t, P]),
        "lf_convchain_plan_create": (P, [I, I, I, I, P, P]),
        "lf_convchain_plan_destroy": (None, [P]),
        "lf_convchain_workspace_bytes": (c_size_t, [P]),
        "lf_convchain_forward": (I, [P, P, P, P, P, I, ctypes.c_float, ctypes.c_float, P, P, c_size_t, P]),
        "lf_convchain_backward": (I, [P, P, P, P, P, P, P, I, P, c_size_t, P]),
        "lf_poolflat_fwd": (I, [P, I, I, I, I, I, P, P]),
        "lf_poolflat_bwd": (I, [P, P, I, I, I, I, I, P, P]),
        "lf_convchain_workspace_bytes_for": (c_size_t, [P, I]),
        "lf_convchain_set_precision": (I, [P, I]),
        "lf_poolflat_bf16_fwd": (I, [P, I, I, I, I, I, P, P]),
        "lf_poolflat_bf16_bwd": (I, [P, P, I, I, I, I, I, P, P]),
        "lf_lane_decode": (I, [P, P, P, P, D, P, P, D, D, D, I, I, I, I, P, P, P]),
        "lf_trapezoid": (I, [P, P, I, D, D, I, I, P, P]),
        "lf_pipeline_plan_create": (P, [I, I, I, I, I, I]),
        "lf_pipeline_plan_destroy": (None, [P]),
        "lf_pipeline_table_bytes": (c_size_t, [P]),
        "lf_pipeline_upload": (I, [P, P, P]),
        "lf_pipeline_tables_host": (I, [P, P, P, P, P, P, P, P, P]),
        "lf_pipeline_image": (I, [P, P, I, P, P, P, P]),
        "lf_pipeline_label": (I, [P, P, I, P, P, I, P, P, P, P]),
        "lf_pipeline_image_indexed": (I, [P, P, L, P, I, P, P, P, P, P]),
        "lf_pipeline_label_indexed": (I, [P, P, L, P, I, P, P, I, P, P, P, P, P]),
        "lf_nhwc_to_nchw": (I, [P, P, I, I, I, I, P]),
        "lf_pointwise_fwd": (I, [P, P, P, P, I, I, I, I, I, P]),
        "lf_pointwise_scratch_floats": (L, [I, I, I, I, I]),
        "lf_pointwise_bwd": (I, [P, P, P, P, P, P, I, I, I, I, I, P, P]),
        "lf_pointwise_bf16_fwd": (I, [P, P, P, P, I, I, I, I, I, P]),
        "lf_pointwise_bf16_bwd": (I, [P, P, P, P, P, P, I, I, I, I, I, P, P]),
        "lf_adam_chunk": (I, []),
        "lf_adam_step": (I, [P, P, I, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                             I, ctypes.c_float, P]),
        "lf_sgd_step": (I, [P, P, I, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, P]),
        "lf_rmsprop_step": (I, [P, P, I, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                ctypes.c_float, P]),
        "lf_conv1d_scratch_floats": (L, [I, I, I, I]),
        "lf_conv1d_fwd": (I, [P, P, P, P, I, I, I, I, I, I, I, P, P]),
        "lf_conv1d_bwd_data": (I, [P, P, P, P, I, I, I, I, I, I, P, P]),
        "lf_conv1d_bwd_weight": (I, [P, P, P, P, I, I, I, I, I, I, P, P]),
        "lf_erfnet_num_layers": (I, [P]),
        "lf_erfnet_range_workspace_bytes": (c_size_t, [P, I, I]),
        "lf_erfnet_layer_io": (I, [P, I, P]),
        "lf_erfnet_forward_range": (I, [P, I, I, I, P, P, P, P, P, I, P, P, c_size_t, P]),
        "lf_erfnet_backward_range": (I, [P, I, I, I, P, P, P, P, P, I, P, P, c_size_t, P]),
        "lf_linear_fwd": (I, [P, P, P, P, I, I, I, I, P]),
        "lf_linear_bwd": (I, [P, P, P, P, P, P, P, I, I, I, I, P]),
        "lf_seg_maps": (I, [P, P, P, I, I, I, I, I, I, P]),
        "lf_erfnet_set_precision": (I, [P, I]),
        "lf_erfnet_profile": (I, [P, I]),
        "lf_erfnet_profile_read": (I, [P, P, c_char_p]),
        "lf_erfnet_infer_workspace_bytes": (c_size_t, [P, I]),
        "lf_erfnet_infer_encoder_offset": (L, [P]),
        "lf_erfnet_infer": (I, [P, P, P, P, P, I, P, P, c_size_t, P]),
        "lf_erfnet_infer_range_workspace_bytes": (c_size_t, [P, I, I, I]),
        "lf_erfnet_infer_range": (I, [P, I, I, I, P, P, P, P, P, P, c_size_t, P]),
        "lf_convchain_infer_workspace_bytes": (c_size_t, [P, I]),
        "lf_convchain_infer": (I, [P, P, P, P, P, ctypes.c_float, P, P, c_size_t, P]),
        "lf_head_fit": (I, [P, I, P, P, P, L, I, I, I, I, I, I, D, D, I, I, P, P, P, P, P, P]),
        "lf_lane_infer_workspace_bytes": (c_size_t, [P, I, I, I]),
        "lf_lane_infer": (I, [P, P, P, P, P, P, L, I, I, D, D, I, I, P, P, P, P, c_size_t, P]),
        "lf_theta_grid": (I, [P, L, P, P, I, I, I, P, P]),
        "lf_theta_grid_bwd_workspace_bytes": (c_size_t, [I]),
        "lf_theta_grid_bwd": (I, [P, L, P, P, P, I, I, I, P, P, P]),
        "lf_wls_fwd_theta": (I, [P, P, L, P, P, I, I, I, I, I, I, D, D, I, I, P, P, P, P, P, P]),
        "lf_wls_bwd_theta_workspace_bytes": (c_size_t, [I, I]),
        "lf_wls_bwd_theta": (I, [P, P, L, P, P, I, I, I, I, I, I, D, I, P, P, P, P, P, P, P]),
        "lf_wls_bwd_grid": (I, [P, P, L, I, I, I, I, I, I, D, I, P, P, P, P, P]),
        "lf_lane_eval": (I, [P, P, P, P, P, P, L, P, I, I, I, I, I, D, D, P, P, P, P, P, P]),
        "lf_lane_decode_bev": (I, [P, I, P, P, P, P, L, P, P, I, D, P, P, I, I, I, I, I, I, I, I, I, I, P, P, P]),
        "lf_step_loss_workspace_bytes": (c_size_t, []),
        "lf_step_loss": (I, [I, I, I, I, I, I, I, P, L, I, P, P, L, I, P, P, P, P, P, P, P, I, D, D, P, P, P, P, P, P]),
        "lf_step_loss_bwd": (I, [P, I, L, L, P, P, P]),
        "lf_seg_step_workspace_bytes": (c_size_t, [I, I, I, I, I, I]),
        "lf_seg_step": (I, [P, P, P, P, L, P, I, I, I, I, I, I, I, D, D, I, P, P, P, P, P, P, P, P]),
        "lf_seg_step_bwd": (I, [P, L, P, P]),
        "lf_label_batch_bp": (I, [P, P, P, P, P, P, P, L, P, P, I, I, P, P, P, P, P, P, P, P, P]),
        "lf_label_batch_bev": (I, [P, P, P, P, P, L, P, P, I, P, P, P, P, P, P, P]),
        "lf_grad_norm_workspace_bytes": (c_size_t, [I]),
        "lf_grad_sumsq": (I, [P, P, I, I, P, P]),
        "lf_grad_norm_finish": (I, [P, I, ctypes.c_float, ctypes.c_float, P, P]),
        "lf_grad_scale_inplace": (I, [P, P, I, ctypes.c_float, P, P]),
        "lf_adam_step_clipped": (I, [P, P, I, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                     I, ctypes.c_float, P, P]),
        "lf_sgd_step_clipped": (I, [P, P, I, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, P, P]),
        "lf_rmsprop_step_clipped": (I, [P, P, I, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                        ctypes.c_float, P, P]),
        "lf_head_fit_seg": (I, [P, I, P, P, P, L, P, I, I, I, I, I, I, I, D, D, I, P, P, P, P, P, P]),
        "lf_lane_infer_seg_workspace_bytes": (c_size_t, [P, I, I, I]),
        "lf_lane_infer_seg": (I, [P, P, P, P, P, P, L, P, I, I, I, D, D, I, P, P, P, P, c_size_t, P]),
        "lf_stem_bwd_data": (I, [P, P, P, I, I, I, I, I, P, P]),
        "lf_erfnet_backward_input": (I, [P, P, P, P, P, P, P, I, I, P, P, c_size_t, P]),
        "lf_erfnet_infer_fold": (I, [P, P, P, P, P, c_size_t, P]),
        "lf_lane_infer_folded": (I, [P, P, P, P, P, P, L, I, I, D, D, I, I, P, P, P, P, c_size_t, I, P]),
        "lf_lane_infer_seg_folded": (I, [P, P, P, P, P, P, L, P, I, I, I, D, D, I, P, P, P, P, c_size_t, I, P]),
        "lf_convchain_infer_fold": (I, [P, P, P, P, ctypes.c_float, P, c_size_t, P]),
        "lf_convchain_infer_folded": (I, [P, P, P, P, c_size_t, I, P]),
        "lf_clas_tail_workspace_bytes": (c_size_t, [I, I, I, I, I]),
        "lf_clas_tail": (I, [P, P, I, I, I, I, I, P, P, I, P, P, P, P, I, P, I, I, P, P, I, P, D, D, D, D, P, P, P, P, P, P,
                             c_size_t, P]),
        "lf_pipeline_frame_stem_ok": (I, [P]),
        "lf_pipeline_frame_stem_lds_bytes": (c_size_t, [P]),
        "lf_pipeline_frame_stem_tile": (I, [P, P, P]),
        "lf_lane_infer_u8_workspace_bytes": (c_size_t, [P, I, I, I]),
        "lf_lane_infer_seg_u8_workspace_bytes": (c_size_t, [P, I, I, I]),
        "lf_lane_infer_folded_u8": (I, [P, P, P, P, P, P, P, P, L, I, I, D, D, I, I, P, P, P, P, c_size_t, I, P]),
        "lf_lane_infer_seg_folded_u8": (I, [P, P, P, P, P, P, P, P, L, P, I, I, I, D, D, I, P, P, P, P, c_size_t, I, P]),
        "lf_pipeline_plan_set_format": (I, [P, I, P]),
        "lf_pipeline_frame_bytes": (c_size_t, [P]),
        "lf_pipeline_plan_set_layout": (I, [P, P, P]),
        "lf_pipeline_surface_span": (c_size_t, [P, I]),
    }
    # test / tooling hooks (csrc/lf_debug.h; not part of include/lanefit.h)
    dbg = {
        "lf_debug_set_split_any_size": (None, [I]),
        "lf_debug_set_bf16_lds": (None, [I]),
        "lf_debug_set_bf16_no_partial_fast": (None, [I]),
        "lf_debug_stride2_epi": (I, [I, I, P, P, P, P, I, P, P, P, P, I, I, I, I, I, P, P]),
        "lf_debug_stride2_wgrad_scratch_floats": (L, [I, I, I, I, I, I, I]),
        "lf_debug_stride2_wgrad": (I, [I, I, P, P, P, P, I, I, I, I, I, P, P]),
        "lf_debug_stem_wgrad_scratch_floats": (L, [I, I, I, I]),
        "lf_debug_stem_wgrad": (I, [I, P, P, P, P, I, I, I, I, P, P]),
        "lf_debug_head_wgrad_scratch_floats": (L, [I, I, I, I]),
        "lf_debug_head_wgrad": (I, [I, P, P, P, P, I, I, I, I, P, P]),
        "lf_debug_set_ops_precision": (None, [I]),
        "lf_debug_conv1d_fwd_phases": (I, [P, P, P, P, I, I, I, I, I, I, P, P, P]),
        "lf_debug_conv1d_wgrad_phases": (I, [P, P, I, I, I, I, I, I, P, P, P]),
        "lf_debug_conv1d_fwd_pro": (I, [P, P, P, P, P, P, I, I, I, I, I, I, P, P]),
        "lf_debug_set_wgrad_ro": (None, [I, I, I]),
        "lf_debug_set_fp32_stream": (None, [I, I]),
        "lf_debug_set_bwd16_fused": (None, [I]),
        "lf_debug_set_fwd_pair": (None, [I, I]),
        "lf_debug_conv1d_fwd_pair": (I, [P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, P, P]),
        "lf_debug_conv1d_bwd_pair_scratch_floats": (L, [I, I, I, I]),
        "lf_debug_conv1d_bwd_pair": (I, [P, P, P, I, P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, P, P]),
        "lf_debug_conv1d_bwd_data_epi3": (I, [P, P, P, P, P, P, P, I, I, I, I, I, I, P, P]),
        "lf_debug_conv1d_epi": (I, [P, P, P, P, I, I, P, P, P, P, P, P, I, I, I, I, I, I, P, P]),
        "lf_debug_conv1d_wgrad_pro": (I, [P, P, P, P, P, P, I, I, I, I, I, I, P, P]),
        "lf_debug_bias_residual_launches": (L, []),
        "lf_debug_partial_fast_launches": (L, []),
        "lf_debug_bf16_ring_launches": (L, []),
        "lf_debug_set_bf16_max_workgroups": (None, [I]),
        "lf_debug_set_thin": (None, [I, I]),
        "lf_debug_thin_launches": (L, []),
        "lf_debug_set_thin_bf16": (None, [I, I]),
        "lf_debug_thin_bf16_launches": (L, []),
        "lf_debug_fold_pack_launches": (L, []),
        # one launch of a bandwidth-bound backbone kernel; a source of partial rows = (rows, nrows, ld, C, ch_off, tile_pix, seg_rows, seg_pix)
        "lf_debug_bn_finalize_fwd": (I, [P, I, I, I, I, I, I, L] * 2 + [I, D, P, P, P, P, ctypes.c_float, ctypes.c_float, I, P, P, P, P, P]),
        "lf_debug_bn_bwd_finalize": (I, [P, I, I, I, I, I, I, L] * 2 + [I, D, P, P, P, P, P, P, I, P]),
        "lf_debug_bn_act": (I, [P, P, P, P, P, P, L, I, L, I, P]),
        "lf_debug_bn_bwd_reduce": (I, [P, P, P, P, P, P, P, I, L, I, L, I, P]),
        "lf_debug_bn_bwd_apply": (I, [P, P, P, P, P, P, P, P, P, P, P, L, I, L, I, P]),
        "lf_debug_pool_concat_fwd": (I, [P, I, I, I, I, P, I, I, P, I, I, P]),
        "lf_debug_pool_affine_fwd": (I, [P, I, I, I, I, P, I, I, P, P, I, P]),
        "lf_debug_pool_bwd": (I, [P, P, I, I, I, I, I, I, P, I, P]),
        "lf_debug_stem_fwd": (I, [P, I, I, I, I, P, P, P, P, P, P, I, I, P]),
        "lf_debug_frame_stem": (I, [P, P, I, P, P, P, P, P, P, I, P]),
        "lf_debug_head_fwd": (I, [P, P, P, P, I, I, I, I, I, P]),
        "lf_debug_head_bwd_data": (I, [P, P, P, I, I, I, I, I, P]),
        "lf_debug_convchain_offset": (L, [P, I, I]),
    }
    for table in (sig, dbg):
        for name, (res, args) in table.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
    return sig


def exported_symbols():
    """Names include/lanefit.h declares (used by the CPU test that checks the .so exports them)."""
    return list(_declare(load()).keys()) + list(_extra_symbols)


# ... and the csrc/lf_debug.h hooks the frozen detector's tests and tools/detector_latency.py count launches with
_extra_symbols = ["lf_debug_set_thin", "lf_debug_thin_launches", "lf_debug_fold_pack_launches", "lf_debug_set_thin_bf16",
                  "lf_debug_thin_bf16_launches", "lf_debug_frame_stem"]


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LaneFitLibraryError(
                "%s not found: build it with `python -m lanedetection_end2end_amd.build` "
                "(there is no fallback path)" % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        _declare(lib)
        _lib = lib
    return _lib


def check(rc, what):
    if rc != 0:
        raise LaneFitLibraryError("%s failed: %s" % (what, load().lf_last_error().decode()))


def ptr(t, rows=False):
    """Device pointer of a contiguous CUDA(HIP) tensor, or None.  rows=True: a 2-D tensor with contiguous ROWS is enough (the
    entry point takes the row stride: beta_stride of the loss kernels)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise LaneFitLibraryError("lanefit ops need tensors on the MI355X (got a %s tensor); "
                                  "there is no CPU path" % t.device)
    if rows:
        assert t.dim() == 2 and t.stride(1) == 1, "internal: tensor rows must be contiguous"
    else:
        assert t.is_contiguous(), "internal: tensor must be contiguous"
    return c_void_p(t.data_ptr())


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


class DeferredRead:
    """A few device scalars read back WITHOUT stalling the stream: the copy to pinned host memory and an event are enqueued
    right behind the kernel / collective that produced them; ``get()`` waits for THAT event only.  (``t.tolist()`` / ``float(t)``
    at a later point enqueue their copy behind everything launched since -- e.g. the whole next forward + backward -- and block
    the host until that finishes: the hidden per-step sync VERDICT round 3 found in the reducer and the cross-entropy check.)
    Host tensors are cloned (the gloo / CPU tests)."""

    def __init__(self, t):
        if t.is_cuda:
            self.host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            self.host.copy_(t, non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record()
        else:
            self.host = t.detach().clone()
            self.event = None

    def ready(self):
        return self.event is None or self.event.query()

    def get(self):
        if self.event is not None:
            self.event.synchronize()
        return self.host
