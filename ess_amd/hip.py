"""
ctypes binding of libess_hip.so (include/ess_hip.h).  This is the only place the C ABI is touched.

The library is built in-tree by ``__graft_entry__.build()`` (hipcc --offload-arch=gfx950).  There is
NO fallback: if the library is missing, or a tensor is not a contiguous fp32 CUDA(HIP) tensor, the
call raises.  PyTorch only supplies device memory and the current HIP stream.
"""
import ctypes
import os
from ctypes import POINTER, Structure, byref, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

import numpy as np
import torch

from . import copies

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libess_hip.so')

SRC_DIRECT, SRC_NEAREST_UP2, SRC_ZERO_UP2, SRC_S2D = 0, 1, 2, 3
EPI_LINEAR, EPI_LSTM, EPI_GRU_UR, EPI_GRU_OUT = 0, 1, 2, 3
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, ACT_SUMPOOL2 = 0, 1, 2, 3, 4
W_CONV, W_TRANSPOSED, W_ROWS, W_CONV5_S2D = 0, 1, 2, 3
GRU_U_F32, GRU_U_F16 = 0, 1
COMPUTE_FP32, COMPUTE_BF16, COMPUTE_BF16X3, COMPUTE_F16 = 0, 1, 2, 3
FMT_F32_NCHW, FMT_BF16_C8, FMT_F32_C8, FMT_F16_C8, FMT_F16_C8_HILO = 0, 1, 2, 3, 4
LSTM_H_HILO = 1
GRU_H_HILO = 2

_default_compute = COMPUTE_FP32
_mixed = False


def set_compute(kind):
    """Arithmetic of the convolution contractions for specs created without an explicit `compute`:
    'fp32' (exact fp32 MFMA; BASELINE config 2), 'bf16' (bf16 MFMA operands, fp32 accumulate, BF16_C8 tensors in the trainable
    networks; BASELINE config 3), or 'bf16x3' (split-operand bf16, ESS_COMPUTE_BF16X3: fp32 tensors exactly as in the 'fp32'
    configuration, every 3x3 / stride-1 contraction -- forward, data-gradient, recurrent gates, weight gradient -- as
    w_hi x_hi + w_hi x_lo + w_lo x_hi on the bf16 matrix cores with fp32 accumulators, ~2^-16 relative operand error; every other
    convolution on the exact-fp32 kernels: the parity-grade configuration at a matrix-core-rate step)."""
    global _default_compute, _mixed
    # 'mixed' (round 6): the bf16 configuration's storage and BACKWARD arithmetic (BF16_C8 tensors, bf16 data- and weight-gradients),
    # every FORWARD contraction of the frozen encoder's recurrent part and of the decoder on IEEE-half operands (ESS_COMPUTE_F16, the
    # same matrix-core rate, 11 instead of 8 significant bits), [hi | lo] half pairs where an operand's mean is large against its
    # spread (the encoder convolution feeding a recurrent block, the event latents, the first decoder layer's pre-norm tensor):
    # per-pixel argmax / mIoU parity with the fp32 reference at the bf16 step's cost + ~15 %
    _mixed = kind == 'mixed'
    if _mixed:
        kind = 'bf16'
    _default_compute = {'fp32': COMPUTE_FP32, 'bf16': COMPUTE_BF16, 'bf16x3': COMPUTE_BF16X3, COMPUTE_FP32: COMPUTE_FP32,
                        COMPUTE_BF16: COMPUTE_BF16, COMPUTE_BF16X3: COMPUTE_BF16X3}[kind]


def get_compute():
    """'fp32' | 'bf16' | 'bf16x3' -- storage / backward arithmetic; the 'mixed' configuration reports 'bf16' here and True from mixed()"""
    return {COMPUTE_FP32: 'fp32', COMPUTE_BF16: 'bf16', COMPUTE_BF16X3: 'bf16x3'}[_default_compute]


def mixed():
    return _mixed


def compute_name():
    """the name set_compute() was given"""
    return 'mixed' if _mixed else get_compute()

EXPORTS = [
    'ess_last_error', 'ess_version', 'ess_conv2d_plan', 'ess_conv2d_pack_weights', 'ess_conv2d_pack_rows',
    'ess_conv2d_forward', 'ess_to_bf16_c8', 'ess_conv2d_wgrad_workspace', 'ess_conv2d_wgrad', 'ess_conv2d_wgrad_sets', 'ess_norm_workspace', 'ess_instnorm_forward',
    'ess_instnorm_backward', 'ess_batchnorm_train_forward', 'ess_batchnorm_train_backward',
    'ess_upsample_bilinear2x_add', 'ess_sumpool2x2', 'ess_add', 'ess_event_normalize', 'ess_task_loss_workspace',
    'ess_task_loss', 'ess_sym_js_loss', 'ess_l1_loss', 'ess_radam_step', 'ess_argmax_confusion', 'ess_resize_nearest', 'ess_conv2d_pack_weights_multi',
    'ess_voxel_grid_trilinear', 'ess_voxel_grid_trilinear_workspace', 'ess_voxel_grid_temporal', 'ess_voxel_normalize_workspace', 'ess_voxel_normalize',
    'ess_from_bf16_c8', 'ess_norm_workspace_c8', 'ess_instnorm_forward_c8', 'ess_instnorm_backward_c8', 'ess_batchnorm_train_forward_c8',
    'ess_batchnorm_train_backward_c8', 'ess_l1_loss_c8', 'ess_augment_image_label', 'ess_radam_step_dev', 'ess_upsample_bilinear2x_add_c8',
    'ess_upsample_bilinear2x_add_c8_from_c8', 'ess_add_bf16', 'ess_event_normalize_slices', 'ess_sum_scalars',
    'ess_label_confusion', 'ess_augment_perspective_filter', 'ess_tuning_set', 'ess_tuning_get', 'ess_conv2d_s2d_preferred',
    'ess_to_f16_c8', 'ess_bf16_c8_to_f16_c8', 'ess_f16_c8_to_bf16_c8', 'ess_instnorm_forward_c8_mixed', 'ess_seg_head',
    'ess_event_normalize_samples', 'ess_state_carry_masked', 'ess_state_carry_indexed',
    'ess_event_ingest_workspace', 'ess_event_ingest', 'ess_event_ingest_columns', 'ess_event_ingest_ring',
    'ess_event_ingest_columns_trilinear', 'ess_event_ingest_ring_trilinear', 'ess_seg_head_eval',
    'ess_event_scatter_ring', 'ess_event_scatter_ring_trilinear', 'ess_event_grid_finish_workspace', 'ess_event_grid_finish',
    'ess_event_grid_finish_window', 'ess_label_window',
    'ess_event_scatter_ring_rep', 'ess_event_ingest_ring_rep', 'ess_event_ingest_columns_rep',
    'ess_event_ingest_masked', 'ess_event_hot_pixel_mask',
    'ess_event_scatter_store', 'ess_event_store_windows',
    'ess_event_ingest_store', 'ess_event_store_pixel_counts', 'ess_event_count_mask',
    'ess_recon_post_frame', 'ess_recon_post_bounds', 'ess_event_preview',
    'ess_recon_post_frame_steered', 'ess_recon_post_bounds_steered',
    'ess_viz_semseg', 'ess_viz_events', 'ess_viz_overlay',
    'ess_image_ingest', 'ess_augment_image_label_store',
    'ess_image_ingest_frame', 'ess_image_gather_unit',
]


class EssConvDesc(Structure):
    _fields_ = [(n, c_int32) for n in (
        'N', 'H_in', 'W_in', 'C0', 'C1', 'mode0', 'mode1', 'C_out', 'H_out', 'W_out', 'ksize', 'stride', 'pad',
        'epilogue', 'act', 'hidden', 'out_split', 'compute', 'fmt0', 'fmt1', 'fmt_out', 'fmt_res')]


class EssConvPlan(Structure):
    _fields_ = [('cout_tile', c_int32), ('ck', c_int32), ('n_chunks', c_int32), ('n_cout_tiles', c_int32),
                ('packed_elems', c_int64), ('packed_bytes', c_int64), ('rows_padded', c_int32), ('lds_bytes', c_int32)]


class EssVizDst(Structure):
    _fields_ = [('plane_stride', c_int64), ('row_stride', c_int64), ('tile_stride_y', c_int64), ('tile_stride_x', c_int64),
                ('tile0', c_int32), ('tiles_per_row', c_int32)]


class EssHipError(RuntimeError):
    pass


_lib = None


def lib():
    """Load libess_hip.so once.  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EssHipError(f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                              '(hipcc --offload-arch=gfx950). ess_amd has no CPU or eager fallback.')
        L = ctypes.CDLL(LIB_PATH)
        L.ess_last_error.restype = c_char_p
        L.ess_conv2d_wgrad_workspace.restype = c_size_t
        L.ess_conv2d_wgrad_workspace.argtypes = [POINTER(EssConvDesc)]
        L.ess_task_loss_workspace.restype = c_size_t
        L.ess_task_loss_workspace.argtypes = [c_int32]
        L.ess_norm_workspace.restype = c_size_t
        L.ess_norm_workspace.argtypes = [c_int32]
        L.ess_norm_workspace_c8.restype = c_size_t
        L.ess_norm_workspace_c8.argtypes = [c_int32]
        L.ess_voxel_normalize_workspace.restype = c_size_t
        L.ess_voxel_normalize_workspace.argtypes = [c_int32]
        L.ess_voxel_grid_trilinear_workspace.restype = c_size_t
        L.ess_voxel_grid_trilinear_workspace.argtypes = [c_int64, c_int32, c_int32, c_int32]
        L.ess_event_ingest_workspace.restype = c_size_t
        L.ess_event_ingest_workspace.argtypes = [c_int32, c_int32, c_int32, c_int32]
        L.ess_event_grid_finish_workspace.restype = c_size_t
        L.ess_event_grid_finish_workspace.argtypes = [c_int32, c_int32, c_int32, c_int32]
        P, F, I, I64 = c_void_p, c_float, c_int32, c_int64
        D = POINTER(EssConvDesc)
        sig = {
            'ess_conv2d_plan': [D, POINTER(EssConvPlan)],
            'ess_conv2d_s2d_preferred': [D],
            'ess_conv2d_pack_weights': [D, c_int, P, P, P, P],
            'ess_conv2d_pack_rows': [D, P, P, F, P, P],
            'ess_conv2d_forward': [D, P, P, P, P, P, P, P, P, P, P, P, P],
            'ess_to_bf16_c8': [P, P, I, I, I, I, P],
            'ess_conv2d_wgrad': [D, P, P, P, P, P, c_int, P, c_size_t, P],
            'ess_conv2d_wgrad_sets': [D, I, P, P, P, P, P, c_int, P, c_size_t, P],
            'ess_instnorm_forward': [P, P, P, P, I, I, F, I, P, c_size_t, P],
            'ess_instnorm_backward': [P, P, P, P, I, I, I, P, c_size_t, P],
            'ess_batchnorm_train_forward': [P, P, P, P, P, P, F, F, P, P, I, I, I, I, P, c_size_t, P],
            'ess_batchnorm_train_backward': [P, P, P, P, P, P, P, P, P, I, I, I, I, I, P, c_size_t, P],
            'ess_upsample_bilinear2x_add': [P, P, P, I, I, I, P],
            'ess_sumpool2x2': [P, P, I, I, I, I, P],
            'ess_add': [P, P, P, I64, P],
            'ess_add_bf16': [P, P, P, P, I64, P],
            'ess_sum_scalars': [P, I, P, P],
            'ess_event_normalize': [P, P, I64, P, P],
            'ess_event_normalize_slices': [P, P, I, I, I64, P, P],
            'ess_task_loss': [P, P, P, P, F, I, I, I, I, I, I, P, c_size_t, P],
            'ess_sym_js_loss': [P, P, P, P, F, I, I, I, P, c_size_t, P],
            'ess_l1_loss': [P, P, P, P, F, I64, P, c_size_t, P],
            'ess_radam_step': [P, P, P, P, I64, F, F, F, F, F, I, P],
            'ess_argmax_confusion': [P, P, P, P, I, I, I, I, P],
            'ess_resize_nearest': [P, P, I, I, I, I, I, P],
            'ess_conv2d_pack_weights_multi': [P, P, P, P, I, P],
            'ess_voxel_grid_trilinear': [P, P, P, P, P, I64, I, I, I, I, P, P, c_size_t, I64, P],
            'ess_voxel_grid_temporal': [P, P, P, P, P, I64, I, I, I, I, I, P, P],
            'ess_voxel_normalize': [P, I, I64, I, P, c_size_t, P],
            'ess_from_bf16_c8': [P, P, I, I, I, I, P],
            'ess_instnorm_forward_c8': [P, P, P, P, I, I, I, F, I, I, P, c_size_t, P],
            'ess_instnorm_backward_c8': [P, P, P, P, I, I, I, I, I, P, c_size_t, P],
            'ess_batchnorm_train_forward_c8': [P, P, P, P, P, P, F, F, P, P, I, I, I, I, I, P, c_size_t, P],
            'ess_batchnorm_train_backward_c8': [P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, P, c_size_t, P],
            'ess_l1_loss_c8': [P, P, P, P, F, I64, I64, P, c_size_t, P],
            'ess_to_f16_c8': [P, P, I, I, I, I, I, P],
            'ess_bf16_c8_to_f16_c8': [P, P, I64, P],
            'ess_f16_c8_to_bf16_c8': [P, P, I, I, I, I, I, P],
            'ess_instnorm_forward_c8_mixed': [P, P, P, P, P, I, I, I, F, I, I, I, P, c_size_t, P],
            'ess_augment_image_label': [P, P, P, P, P, P, I, I, I, I, I, P],
            'ess_radam_step_dev': [P, P, P, P, I64, F, F, F, P, P],
            'ess_upsample_bilinear2x_add_c8': [P, P, P, I, I, I, I, P],
            'ess_upsample_bilinear2x_add_c8_from_c8': [P, P, P, I, I, I, I, P],
            'ess_seg_head': [P, I, P, P, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, P],
            'ess_seg_head_eval': [P, I, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P],
            'ess_event_normalize_samples': [P, P, I, I64, P, P, P],
            'ess_state_carry_masked': [P, P, P, I, I, P, P],
            'ess_state_carry_indexed': [P, P, P, I, I, I, I, P, P, P],
            'ess_event_ingest': [P, P, I64, I, I, I, I, P, c_size_t, P, P],
            'ess_event_ingest_columns': [P, P, P, P, P, P, I64, I, I, I, I, P, c_size_t, P, P],
            'ess_event_ingest_ring': [P, P, P, P, P, P, P, P, I64, I, I, I, I, I, P, c_size_t, P, P],
            'ess_event_ingest_columns_trilinear': [P, P, P, P, P, P, I64, I, I, I, I, P, c_size_t, P, P, P, I, I, I, P],
            'ess_event_ingest_ring_trilinear': [P, P, P, P, P, P, P, P, I64, I, I, I, I, I, P, c_size_t, P, P, P, I, I, I, P],
            'ess_event_scatter_ring': [P, P, P, P, P, P, P, P, I64, I, I, I, I, I, P, c_size_t, P],
            'ess_event_scatter_ring_trilinear': [P, P, P, P, P, P, P, P, I64, I, I, I, I, I, P, c_size_t, P, P, I, I, I, P],
            'ess_event_grid_finish': [P, I, I, I, I, P, c_size_t, I, I, I, I, I, P, P, c_size_t, P],
            'ess_event_grid_finish_window': [P, I, I, I, I, P, c_size_t, I, I, I, I, I, P, I, I, I, P, P, c_size_t, P],
            'ess_label_window': [P, I, I, I, I, I, P, I, I, P, P],
            'ess_event_scatter_ring_rep': [P, P, P, P, P, P, P, P, I64, I, I, I, I, I, P, c_size_t, I, P],
            'ess_event_ingest_ring_rep': [P, P, P, P, P, P, P, P, I64, I, I, I, I, I, P, c_size_t, P, I, P],
            'ess_event_ingest_columns_rep': [P, P, P, P, P, P, I64, I, I, I, I, P, c_size_t, P, I, P],
            'ess_event_ingest_masked': [P, P, P, P, P, P, P, P, I64, I, I, I, I, I, P, c_size_t, P, I, I, P, P, I, I, I, P, P, I, I, I, P],
            'ess_event_hot_pixel_mask': [P, I, I, I, P, P, I, P],
            'ess_event_scatter_store': [P, P, P, P, P, P, P, I64, I64, I64, I, I, I, I, P, c_size_t, I, P, P, I, I, I, P],
            'ess_event_store_windows': [P, I64, I64, P, I, P, P, P, I, I, I, I64, I64, P, P, P, P, P, P],
            'ess_event_ingest_store': [P, P, P, P, P, P, P, I64, I64, I64, I, I, I, I, P, c_size_t, P, I, P, P, I, I, I, P, P, I, I, I, P],
            'ess_event_store_pixel_counts': [P, P, I64, I64, P, P, P, I, I, I, P, P],
            'ess_event_count_mask': [P, I, I, I, P, P, I, P],
            'ess_recon_post_frame': [P, P, F, F, P, P, P, I, I, I, I, I, I, I, P],
            'ess_recon_post_bounds': [P, P, F, F, I, I, I, P, c_size_t, P, P, I, P, P],
            'ess_recon_post_frame_steered': [P, P, F, F, P, P, P, I, I, I, I, I, I, I, P, P],
            'ess_recon_post_bounds_steered': [P, P, F, F, I, I, I, P, c_size_t, P, P, I, I, P, P, P, P],
            'ess_event_preview': [P, P, I, I, I, I, I, I, P],
            'ess_viz_semseg': [P, I, P, P, c_size_t, POINTER(EssVizDst), I, I, I, I, I, P],
            'ess_viz_events': [P, P, c_size_t, POINTER(EssVizDst), I, I, I, I, I, I, P],
            'ess_viz_overlay': [P, P, P, P, I, I, I, I, F, P],
            'ess_image_ingest': [P, I, I, I, P, I, P, I, P, P, I, I, I, P, P, P, P, P, P],
            'ess_augment_image_label_store': [P, P, P, I, I, I, I, P, P, P, P, I, I, I, P],
            'ess_image_ingest_frame': [P, I, I, I, P, I, P, I, P, P, I, I, I, I, P],
            'ess_image_gather_unit': [P, I64, I, I, P, I, I, P, P],
        }
        for name, argtypes in sig.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = c_int
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise EssHipError(f'{what} failed (rc={rc}): {lib().ess_last_error().decode()}')


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t, dtype=torch.float32, allow_none=True):
    """Device pointer of a contiguous CUDA tensor (or NULL)."""
    if t is None:
        if not allow_none:
            raise EssHipError('required tensor is None')
        return c_void_p(0)
    if not t.is_cuda:
        raise EssHipError('ess_amd kernels need CUDA(HIP) tensors; there is no CPU path (got a CPU tensor)')
    if t.dtype != dtype:
        raise EssHipError(f'expected {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise EssHipError('expected a contiguous tensor')
    return c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------ conv
_desc_cache = {}


class ConvSpec:
    """Descriptor + plan of one convolution shape (cached)."""

    def __init__(self, key):
        (N, H_in, W_in, C0, C1, mode0, mode1, C_out, k, s, p, epi, act, hidden, out_split, compute) = key
        H_out = (H_in + 2 * p - k) // s + 1
        W_out = (W_in + 2 * p - k) // s + 1
        self.desc = EssConvDesc(N, H_in, W_in, C0, C1, mode0, mode1, C_out, H_out, W_out, k, s, p, epi, act, hidden,
                                out_split, compute, FMT_F32_NCHW, FMT_F32_NCHW, FMT_F32_NCHW, FMT_F32_NCHW)
        self._desc_fmt = {}
        self.plan = EssConvPlan()
        _check(lib().ess_conv2d_plan(byref(self.desc), byref(self.plan)), 'ess_conv2d_plan')
        self.key = key
        self.H_out, self.W_out = H_out, W_out
        self.wgrad_ws = None

    def desc_fmt(self, src_fmt=FMT_F32_NCHW, out_fmt=FMT_F32_NCHW, res_fmt=FMT_F32_NCHW):
        """The same convolution (same plan, same packed weights) with the given storage formats of the sources, of the
        output(s) and of the residual."""
        key = (src_fmt, out_fmt, res_fmt)
        d = self._desc_fmt.get(key)
        if d is None:
            d = EssConvDesc.from_buffer_copy(self.desc)
            d.fmt0 = d.fmt1 = src_fmt
            d.fmt_out, d.fmt_res = out_fmt, res_fmt
            self._desc_fmt[key] = d
        return d

    def desc_c8(self):
        """The same convolution reading BF16_C8 sources."""
        return self.desc_fmt(FMT_BF16_C8)


def conv_spec(N, H_in, W_in, C0, C1, C_out, k, s, p, mode0=SRC_DIRECT, mode1=SRC_DIRECT, epi=EPI_LINEAR, act=ACT_NONE,
              hidden=0, out_split=0, compute=None):
    if compute is None:
        compute = _default_compute
    key = (N, H_in, W_in, C0, C1, mode0, mode1, C_out, k, s, p, epi, act, hidden, out_split, compute)
    sp = _desc_cache.get(key)
    if sp is None:
        sp = _desc_cache[key] = ConvSpec(key)
    return sp


def s2d_preferred(spec):
    """Is the space-to-depth form (an ESS_SRC_S2D spec) the faster way to run its 5x5 / stride-2 convolution on this device?  (cached)"""
    v = getattr(spec, '_s2d_pref', None)
    if v is None:
        v = spec._s2d_pref = bool(lib().ess_conv2d_s2d_preferred(byref(spec.desc)))
    return v


def spec_of(key):
    """The cached ConvSpec of a `conv_spec` key tuple."""
    sp = _desc_cache.get(key)
    if sp is None:
        sp = _desc_cache[key] = ConvSpec(key)
    return sp


def pack_weights(spec, w, w2=None, kind=W_CONV):
    out = torch.empty(spec.plan.packed_bytes, dtype=torch.uint8, device=w.device)
    _check(lib().ess_conv2d_pack_weights(byref(spec.desc), kind, ptr(w), ptr(w2), c_void_p(out.data_ptr()), stream()),
           'ess_conv2d_pack_weights')
    return out


def pack_weights_multi(jobs):
    """Re-pack many weights in one launch.  jobs: list of (spec, kind, weight, packed buffer); kind W_ROWS: `weight` is a bias vector
    and the buffer the fp32 one pack_rows() returned.  Raises EssHipError when a job is not a plain bf16 LINEAR layout (nothing is
    launched then)."""
    n = len(jobs)
    descs = (EssConvDesc * n)(*[j[0].desc for j in jobs])
    kinds = (c_int32 * n)(*[int(j[1]) for j in jobs])
    ws = (c_void_p * n)(*[ptr(j[2]).value for j in jobs])
    outs = (c_void_p * n)(*[j[3].data_ptr() for j in jobs])
    _check(lib().ess_conv2d_pack_weights_multi(descs, kinds, ws, outs, n, stream()), 'ess_conv2d_pack_weights_multi')


def pack_rows(spec, v, v2=None, fill=0.0):
    out = torch.empty(spec.plan.rows_padded, dtype=torch.float32, device=v.device)
    _check(lib().ess_conv2d_pack_rows(byref(spec.desc), ptr(v), ptr(v2), c_float(fill), ptr(out), stream()),
           'ess_conv2d_pack_rows')
    return out


def conv_forward(spec, src0, src1, packed_w, scale=None, shift=None, residual=None, aux0=None, aux1=None, out=None,
                 out2=None, out_bf=None, src_fmt=FMT_F32_NCHW, out_fmt=FMT_F32_NCHW, aux_fmt=FMT_F32_NCHW):
    """src_fmt FMT_BF16_C8: src0/src1 are bf16 [N][C/8][H][W][8] tensors (see bf16_c8_empty);
    LSTM epilogue: out_fmt / aux_fmt FMT_F32_C8: out, out2 / aux0 are fp32 [N][hid/8][H][W][8] state tensors (f32_c8_empty);
    out_bf: additionally receives `out` in that format (the frozen encoder's staging copies);
    out_fmt FMT_BF16_C8: `out` / `out2` (and `residual`, if any) ARE BF16_C8 tensors, no fp32 tensor is written."""
    if is_f16_c8(src0) or is_f16_c8(src1) or is_f16_c8(residual):
        raise EssHipError('conv_forward: an F16_C8 (pre-norm) tensor is read by the norm kernels only, not as a BF16_C8 source / residual')
    if out_fmt == FMT_F16_C8 and not is_f16_c8(out):
        raise EssHipError('conv_forward: an F16_C8 output must come from f16_c8_empty (the tag is how its consumers know the format)')
    sdt = torch.bfloat16 if src_fmt == FMT_BF16_C8 else torch.float32
    odt = torch.bfloat16 if out_fmt in (FMT_BF16_C8, FMT_F16_C8) else torch.float32  # (an F16_C8 tensor travels in a bfloat16-typed container: see f16_c8_empty)
    rdt = torch.bfloat16 if out_fmt in (FMT_BF16_C8, FMT_F16_C8) else torch.float32  # (an F16_C8 output takes a BF16_C8 residual)
    res_fmt = aux_fmt if aux_fmt != FMT_F32_NCHW else ((FMT_BF16_C8 if out_fmt == FMT_F16_C8 else out_fmt) if residual is not None else FMT_F32_NCHW)
    desc = spec.desc if (src_fmt, out_fmt, res_fmt) == (FMT_F32_NCHW,) * 3 else spec.desc_fmt(src_fmt, out_fmt, res_fmt)
    # ConvGRU with ESS_GRU_U_F16 and channel-blocked states: the update gate (out of GRU_UR, aux1 of GRU_OUT) is an IEEE-half tensor
    u16 = spec.desc.act == GRU_U_F16 and spec.desc.epilogue in (EPI_GRU_UR, EPI_GRU_OUT)
    udt_out = torch.float16 if (u16 and spec.desc.epilogue == EPI_GRU_UR and out_fmt == FMT_F32_C8) else odt
    udt_aux = torch.float16 if (u16 and spec.desc.epilogue == EPI_GRU_OUT and res_fmt == FMT_F32_C8) else torch.float32
    _check(lib().ess_conv2d_forward(byref(desc), ptr(src0, sdt), ptr(src1, sdt),
                                    ptr(packed_w, torch.uint8), ptr(scale), ptr(shift), ptr(residual, rdt), ptr(aux0), ptr(aux1, udt_aux),
                                    ptr(out, udt_out), ptr(out2, odt), ptr(out_bf, torch.bfloat16), stream()),
           'ess_conv2d_forward')
    return out


def c8_stageable(ksize, stride, pad):
    """Can a bf16 convolution of this geometry stage BF16_C8 sources?  1x1 and 3x3 always (wave-specialised or generic tile
    kernel); 5x5 on the tap-paired kernel only, which can be switched off for diagnostics (ESS_CONV_PAIR=0)."""
    if ksize in (1, 3):
        return True
    if ksize == 5:
        return os.environ.get('ESS_CONV_PAIR', '1')[:1] != '0'
    return False


def bf16_c8_empty(N, C, H, W, device):
    """Uninitialised BF16_C8 tensor for a logical [N, C, H, W] activation: bf16 [N][ceil(C/8)][H][W][8]."""
    return torch.empty(N, (C + 7) // 8, H, W, 8, dtype=torch.bfloat16, device=device)


def f16_c8_raw_empty(N, C, H, W, device):
    """Uninitialised IEEE-half [N][ceil(C/8)][H][W][8] tensor that only kernels read (ConvGRU: the update gate between its two
    launches, ESS_GRU_U_F16)."""
    return torch.empty(N, (C + 7) // 8, H, W, 8, dtype=torch.float16, device=device)


def f32_c8_empty(N, C, H, W, device):
    """Uninitialised FMT_F32_C8 tensor (ConvLSTM states between time steps): fp32 [N][ceil(C/8)][H][W][8]."""
    return torch.empty(N, (C + 7) // 8, H, W, 8, dtype=torch.float32, device=device)


def to_bf16_c8(x):
    """fp32 NCHW -> BF16_C8 on the device (round to nearest even, tail channels zero)."""
    N, C, H, W = x.shape
    y = bf16_c8_empty(N, C, H, W, x.device)
    _check(lib().ess_to_bf16_c8(ptr(x), ptr(y, torch.bfloat16), N, C, H, W, stream()), 'ess_to_bf16_c8')
    return y


def from_bf16_c8(y, C):
    """BF16_C8 -> fp32 NCHW on the device (exact)."""
    N, nb, H, W, _ = y.shape
    if is_f16_c8(y):
        raise EssHipError('from_bf16_c8: the tensor holds IEEE half elements (F16_C8): use f16_c8_to_float')
    if not 0 < C <= nb * 8:
        raise EssHipError(f'from_bf16_c8: {C} channels do not fit {nb} blocks')
    x = torch.empty(N, C, H, W, dtype=torch.float32, device=y.device)
    _check(lib().ess_from_bf16_c8(ptr(y, torch.bfloat16), ptr(x), N, C, H, W, stream()), 'ess_from_bf16_c8')
    return x


def is_c8(t):
    """Is `t` a BF16_C8 tensor (bfloat16 [N][C/8][H][W][8])?"""
    return t is not None and t.dtype == torch.bfloat16 and t.dim() == 5 and t.shape[-1] == 8


def f16_c8_empty(N, C, H, W, device):
    """Uninitialised F16_C8 tensor (a pre-normalisation convolution output of the bf16 configuration: IEEE half elements in the
    BF16_C8 layout, read by the norm kernels only).  The container is a BFLOAT16-typed torch tensor on purpose: autograd casts a
    gradient to the dtype of the tensor it belongs to, and the gradient of a pre-norm tensor is a BF16_C8 tensor -- a float16-typed
    container would make the engine insert dtype casts.  The format travels as an explicit flag (conv out_fmt, norm x_f16)."""
    t = torch.empty(N, (C + 7) // 8, H, W, 8, dtype=torch.bfloat16, device=device)
    t.ess_f16 = True  # (python attribute: survives autograd.Function outputs; `is_f16_c8` reads it, the BF16_C8 consumers refuse it)
    return t


def is_f16_c8(t):
    """Was `t` created by f16_c8_empty (IEEE half elements in a bfloat16-typed BF16_C8-shaped container)?"""
    return t is not None and getattr(t, 'ess_f16', False)


def f16_c8_to_float(t, C):
    """fp32 NCHW values of an F16_C8 tensor (tests / diagnostics; plain torch ops)."""
    N, nb, H, W, _ = t.shape
    return t.view(torch.float16).float().permute(0, 1, 4, 2, 3).reshape(N, nb * 8, H, W)[:, :C].contiguous()


_ws_cache = {}


def workspace(nbytes, device, tag='ws', zero=False):
    """Grow-only scratch buffer per (device, stream, tag): kernels on one stream are ordered, so reuse is safe.
    zero: zero-filled when (re)allocated -- for kernels that keep an arrival counter in it and leave it zero themselves."""
    key = (device.index, torch.cuda.current_stream().cuda_stream, tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = (torch.zeros if zero else torch.empty)(max(int(nbytes), 1024), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


LOSS_WORKSPACE_BYTES = 8 * (1 + 2048)  # ESS_LOSS_WORKSPACE_BYTES of include/ess_hip.h: one partial per workgroup


def _mean_loss_ws(device):
    """Workspace of the mean losses (ess_sym_js_loss / ess_l1_loss / ess_l1_loss_c8): one partial per workgroup, written in full by
    every call."""
    return workspace(LOSS_WORKSPACE_BYTES, device, 'mean_loss')


def _wgrad_call(spec, src0, dy):
    """-> (descriptor, element type of X, element type of dY, workspace) of a weight-gradient call.  The storage formats are taken
    from the tensors: BF16_C8 (bfloat16, 5-D) or fp32 NCHW for the sources and for dy."""
    sfmt = FMT_BF16_C8 if is_c8(src0) else FMT_F32_NCHW
    dfmt = FMT_BF16_C8 if is_c8(dy) else FMT_F32_NCHW
    desc = spec.desc if (sfmt, dfmt) == (FMT_F32_NCHW, FMT_F32_NCHW) else spec.desc_fmt(sfmt, dfmt)
    sdt = torch.bfloat16 if sfmt == FMT_BF16_C8 else torch.float32
    ddt = torch.bfloat16 if dfmt == FMT_BF16_C8 else torch.float32
    nbytes = lib().ess_conv2d_wgrad_workspace(byref(desc))
    if nbytes == 0:
        raise EssHipError('ess_conv2d_wgrad_workspace: ' + lib().ess_last_error().decode())
    return desc, sdt, ddt, workspace(nbytes, dy.device, 'wgrad')


def wgrad_workspace(spec, src0, dy):
    """The cached buffer a weight-gradient call of `spec` on these tensors takes its split-K slabs (and split-operand copies) from.
    Every call writes what it reads of it; the tests fill it with NaN bytes before a launch to prove that."""
    return _wgrad_call(spec, src0, dy)[3]


def conv_wgrad(spec, src0, src1, dy, dw, db=None, accumulate=False):
    """dw (+)= the weight gradient of `spec` from the sources and dy (fp32 NCHW or BF16_C8 tensors), db (+)= the bias gradient."""
    desc, sdt, ddt, ws = _wgrad_call(spec, src0, dy)
    _check(lib().ess_conv2d_wgrad(byref(desc), ptr(src0, sdt), ptr(src1, sdt), ptr(dy, ddt), ptr(dw), ptr(db), int(accumulate),
                                  c_void_p(ws.data_ptr()), c_size_t(ws.numel()), stream()), 'ess_conv2d_wgrad')


def conv_wgrad_sets(spec, sets, dw, db=None, accumulate=False):
    """dw (+)= sum over `sets` = [(src0, src1, dy), ...] (1..3 sets of the same convolution, same formats): BF16_C8 3x3 / stride-1 layers
    take ONE launch for all sets (ess_conv2d_wgrad_sets), anything else one accumulating launch per set."""
    src0, _, dy = sets[0]
    for (a0, a1, g) in sets:
        if is_c8(a0) != is_c8(src0) or is_c8(g) != is_c8(dy) or a0.shape != src0.shape or g.shape != dy.shape:
            raise EssHipError('conv_wgrad_sets: the sets must agree in shapes and storage formats')
    desc, sdt, ddt, ws = _wgrad_call(spec, src0, dy)
    n = len(sets)
    a0s = (c_void_p * n)(*[ptr(t[0], sdt).value for t in sets])
    a1s = (c_void_p * n)(*[(ptr(t[1], sdt).value if t[1] is not None else None) for t in sets])
    gs = (c_void_p * n)(*[ptr(t[2], ddt).value for t in sets])
    _check(lib().ess_conv2d_wgrad_sets(byref(desc), n, a0s, a1s, gs, ptr(dw), ptr(db), int(accumulate), c_void_p(ws.data_ptr()),
                                       c_size_t(ws.numel()), stream()), 'ess_conv2d_wgrad_sets')


# ------------------------------------------------------------------------------------------ norms
def instnorm_forward(x, residual, relu, eps=1e-5):
    N, C, H, W = x.shape
    y = torch.empty_like(x)
    stats = torch.empty(N * C, 2, dtype=torch.float32, device=x.device)
    ws = workspace(lib().ess_norm_workspace(N * C), x.device, 'norm')
    _check(lib().ess_instnorm_forward(ptr(x), ptr(residual), ptr(y), ptr(stats), N * C, H * W, c_float(eps), int(relu),
                                      c_void_p(ws.data_ptr()), c_size_t(ws.numel()), stream()), 'ess_instnorm_forward')
    return y, stats


def instnorm_backward(x, dy, stats, relu):
    N, C, H, W = x.shape
    dx = torch.empty_like(x)
    ws = workspace(lib().ess_norm_workspace(N * C), x.device, 'norm')
    _check(lib().ess_instnorm_backward(ptr(x), ptr(dy), ptr(stats), ptr(dx), N * C, H * W, int(relu),
                                       c_void_p(ws.data_ptr()), c_size_t(ws.numel()), stream()), 'ess_instnorm_backward')
    return dx


def batchnorm_train_forward(x, residual, gamma, beta, running_mean, running_var, momentum, eps, relu):
    N, C, H, W = x.shape
    y = torch.empty_like(x)
    stats = torch.empty(C, 2, dtype=torch.float32, device=x.device)
    ws = workspace(lib().ess_norm_workspace(C), x.device, 'norm')
    _check(lib().ess_batchnorm_train_forward(ptr(x), ptr(residual), ptr(gamma), ptr(beta), ptr(running_mean),
                                             ptr(running_var), c_float(momentum), c_float(eps), ptr(y), ptr(stats), N, C,
                                             H * W, int(relu), c_void_p(ws.data_ptr()), c_size_t(ws.numel()), stream()),
           'ess_batchnorm_train_forward')
    return y, stats


def batchnorm_train_backward(x, y, dy, gamma, stats, relu, need_dx=True, need_dres=False, dgamma=None, dbeta=None,
                             accumulate=False):
    N, C, H, W = x.shape
    dx = torch.empty_like(x) if need_dx else None
    dres = torch.empty_like(x) if need_dres else None
    ws = workspace(lib().ess_norm_workspace(C), x.device, 'norm')
    _check(lib().ess_batchnorm_train_backward(ptr(x), ptr(y), ptr(dy), ptr(gamma), ptr(stats), ptr(dx), ptr(dres),
                                              ptr(dgamma), ptr(dbeta), int(accumulate), N, C, H * W, int(relu),
                                              c_void_p(ws.data_ptr()), c_size_t(ws.numel()), stream()),
           'ess_batchnorm_train_backward')
    return dx, dres


# ---- the same norms on BF16_C8 tensors [N, ceil(C/8), H, W, 8] (C = real channel count); x may be an F16_C8 tensor (is_f16c8)
def instnorm_forward_c8(x, C, residual, relu, eps=1e-5, x_f16=False):
    N, CB, H, W, _ = x.shape
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    stats = torch.empty(N * C, 2, dtype=torch.float32, device=x.device)
    L = lib()
    xdt, xf = torch.bfloat16, int(bool(x_f16))
    ws = workspace(L.ess_norm_workspace_c8(N * CB), x.device, 'norm8')
    _check(L.ess_instnorm_forward_c8(ptr(x, xdt), ptr(residual, torch.bfloat16), ptr(y, torch.bfloat16), ptr(stats), N, C,
                                     H * W, c_float(eps), int(relu), xf, c_void_p(ws.data_ptr()), c_size_t(ws.numel()), stream()),
           'ess_instnorm_forward_c8')
    return y, stats


def instnorm_backward_c8(x, C, dy, stats, relu, x_f16=False):
    """x_f16: False / 0 BF16_C8, True / 1 F16_C8, 2 a [hi | lo] half pair [N][2 CB][H][W][8] (its hi parts are read)"""
    N, CB, H, W, _ = x.shape
    if int(x_f16) == 2:
        CB //= 2
    dx = torch.empty(N, CB, H, W, 8, dtype=torch.bfloat16, device=x.device)
    L = lib()
    xdt, xf = x.dtype, int(x_f16)
    ws = workspace(L.ess_norm_workspace_c8(N * CB), x.device, 'norm8')
    _check(L.ess_instnorm_backward_c8(ptr(x, xdt), ptr(dy, torch.bfloat16), ptr(stats), ptr(dx, torch.bfloat16), N, C, H * W,
                                      int(relu), xf, c_void_p(ws.data_ptr()), c_size_t(ws.numel()), stream()), 'ess_instnorm_backward_c8')
    return dx


def batchnorm_train_forward_c8(x, C, residual, gamma, beta, running_mean, running_var, momentum, eps, relu, x_f16=False):
    N, CB, H, W, _ = x.shape
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    stats = torch.empty(2, C, 2, dtype=torch.float32, device=x.device)  # (mean, rstd) pairs, then the forward's (a, b) map
    L = lib()
    xdt, xf = torch.bfloat16, int(bool(x_f16))
    ws = workspace(L.ess_norm_workspace_c8(CB), x.device, 'norm8')
    _check(L.ess_batchnorm_train_forward_c8(ptr(x, xdt), ptr(residual, torch.bfloat16), ptr(gamma), ptr(beta),
                                            ptr(running_mean), ptr(running_var), c_float(momentum), c_float(eps),
                                            ptr(y, torch.bfloat16), ptr(stats), N, C, H * W, int(relu), xf, c_void_p(ws.data_ptr()),
                                            c_size_t(ws.numel()), stream()), 'ess_batchnorm_train_forward_c8')
    return y, stats


def batchnorm_train_backward_c8(x, C, y, dy, gamma, stats, relu, need_dx=True, need_dres=False, dgamma=None, dbeta=None,
                                accumulate=False, x_f16=False, beta=None):
    """beta (with relu, a forward WITHOUT residual): the ReLU mask is recomputed from x with the affine map the forward saved
    in `stats` (the pointer only selects the form; gamma / beta may have changed since the forward), y is not read."""
    if stats.numel() != 4 * C:
        raise EssHipError(f'batchnorm_train_backward_c8: stats must be the forward\'s [2, C, 2] tensor, got {tuple(stats.shape)}')
    N, CB, H, W, _ = x.shape
    dx = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if need_dx else None
    dres = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if need_dres else None
    L = lib()
    xdt, xf = torch.bfloat16, int(bool(x_f16))
    ws = workspace(L.ess_norm_workspace_c8(CB), x.device, 'norm8')
    _check(L.ess_batchnorm_train_backward_c8(ptr(x, xdt), ptr(y, torch.bfloat16), ptr(dy, torch.bfloat16), ptr(gamma), ptr(beta),
                                             ptr(stats), ptr(dx, torch.bfloat16), ptr(dres, torch.bfloat16), ptr(dgamma), ptr(dbeta),
                                             int(accumulate), N, C, H * W, int(relu), xf, c_void_p(ws.data_ptr()), c_size_t(ws.numel()),
                                             stream()), 'ess_batchnorm_train_backward_c8')
    return dx, dres


# ------------------------------------------------------------------------------------------ glue
def _same_shape(what, name, t, shape):
    """Refuse a second operand / destination of another shape before any pointer is taken: the kernels index it with the first
    operand's extents, so a smaller one would be read or written past its end."""
    if t is not None and tuple(t.shape) != tuple(shape):
        raise EssHipError(f'{what}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}')


def upsample_bilinear2x_add(a, b=None):
    N, C, H, W = a.shape
    _same_shape('upsample_bilinear2x_add', 'b', b, a.shape)
    y = torch.empty(N, C, 2 * H, 2 * W, dtype=torch.float32, device=a.device)
    _check(lib().ess_upsample_bilinear2x_add(ptr(a), ptr(b), ptr(y), N * C, H, W, stream()), 'ess_upsample_bilinear2x_add')
    return y


def upsample_bilinear2x_add_c8(a, b=None):
    """bilinear_x2(a + b) written as a BF16_C8 tensor (the staging form of a following bf16 convolution)."""
    N, C, H, W = a.shape
    _same_shape('upsample_bilinear2x_add_c8', 'b', b, a.shape)
    y = bf16_c8_empty(N, C, 2 * H, 2 * W, a.device)
    _check(lib().ess_upsample_bilinear2x_add_c8(ptr(a), ptr(b), ptr(y, torch.bfloat16), N, C, H, W, stream()),
           'ess_upsample_bilinear2x_add_c8')
    return y


def upsample_bilinear2x_add_c8_from_c8(a8, b8=None):
    """bilinear_x2(a + b) from BF16_C8 sources to a BF16_C8 tensor."""
    N, CB, H, W, _ = a8.shape
    _same_shape('upsample_bilinear2x_add_c8_from_c8', 'b8', b8, a8.shape)
    y = torch.empty(N, CB, 2 * H, 2 * W, 8, dtype=torch.bfloat16, device=a8.device)
    _check(lib().ess_upsample_bilinear2x_add_c8_from_c8(ptr(a8, torch.bfloat16), ptr(b8, torch.bfloat16), ptr(y, torch.bfloat16), N,
                                                        CB * 8, H, W, stream()), 'ess_upsample_bilinear2x_add_c8_from_c8')
    return y


def sumpool2x2(x, out=None, accumulate=False):
    N, C, H, W = x.shape
    if H % 2 or W % 2:  # (the kernels stride the input by 2 W_out: an odd W would pool the wrong pixels, an odd H drop a row)
        raise EssHipError(f'sumpool2x2: input extents {H} x {W} must both be even')
    _same_shape('sumpool2x2', 'out', out, (N, C, H // 2, W // 2))
    if out is None:
        out = torch.empty(N, C, H // 2, W // 2, dtype=torch.float32, device=x.device)
    _check(lib().ess_sumpool2x2(ptr(x), ptr(out), N * C, H // 2, W // 2, int(accumulate), stream()), 'ess_sumpool2x2')
    return out


def add(a, b, out=None):
    _same_shape('add', 'b', b, a.shape)
    _same_shape('add', 'out', out, a.shape)
    if out is None:
        out = torch.empty_like(a)
    _check(lib().ess_add(ptr(a), ptr(b), ptr(out), a.numel(), stream()), 'ess_add')
    return out


def add_bf16(a, b, c=None, out=None):
    """a + b (+ c) over bfloat16 tensors of one shape (BF16_C8 gradients): fp32 sum, one rounding."""
    if a.shape != b.shape or (c is not None and c.shape != a.shape) or a.numel() % 8:
        raise EssHipError('add_bf16: shape mismatch / not a whole number of 8-element vectors')
    if out is None:
        out = torch.empty_like(a)
    bf = torch.bfloat16
    _check(lib().ess_add_bf16(ptr(a, bf), ptr(b, bf), ptr(c, bf), ptr(out, bf), a.numel() // 8, stream()), 'ess_add_bf16')
    return out


def sum_scalars(terms):
    """Sum of 0-dim fp32 device tensors (<= 16), in the order given, as one launch."""
    terms = [t.detach() for t in terms]
    out = torch.empty((), dtype=torch.float32, device=terms[0].device)
    arr = (c_void_p * len(terms))(*[ptr(t).value for t in terms])
    _check(lib().ess_sum_scalars(arr, len(terms), ptr(out), stream()), 'ess_sum_scalars')
    return out


def event_normalize(x):
    ptr(x)  # device / dtype / layout check before anything is allocated
    y = torch.empty_like(x)
    ws = workspace(64, x.device, 'evnorm')
    _check(lib().ess_event_normalize(ptr(x), ptr(y), x.numel(), c_void_p(ws.data_ptr()), stream()), 'ess_event_normalize')
    return y


def event_normalize_slices(x, T):
    """EventPreprocessor's normalisation of every time slice x[:, t*C:(t+1)*C] of an event tensor [B, T*C, H, W] in one reduce +
    one map launch -> [T, B, C, H, W] (slice t contiguous); statistics per slice over the whole batch."""
    ptr(x)
    B, TC, H, W = x.shape
    if TC % T:
        raise EssHipError(f'event_normalize_slices: {TC} channels are not {T} equal slices')
    C = TC // T
    y = torch.empty(T, B, C, H, W, dtype=torch.float32, device=x.device)
    ws = workspace(24 * T, x.device, 'evnorm_slices')
    _check(lib().ess_event_normalize_slices(ptr(x), ptr(y), B, T, C * H * W, c_void_p(ws.data_ptr()), stream()), 'ess_event_normalize_slices')
    return y


def _stream_modes(mode, S, what):
    """the per-stream mode words of a batched call: a contiguous int32 [S] device tensor"""
    if not torch.is_tensor(mode) or not mode.is_cuda:
        raise EssHipError(f'{what}: mode must be a CUDA(HIP) int32 tensor; there is no CPU path')
    if mode.dtype != torch.int32 or tuple(mode.shape) != (S,) or not mode.is_contiguous():
        raise EssHipError(f'{what}: mode must be a contiguous int32 [{S}] tensor, got {mode.dtype}{tuple(mode.shape)}')
    return mode


def event_normalize_samples(x, mode=None, out=None):
    """EventPreprocessor's normalisation per SAMPLE of x [S, C, H, W] (S independent event streams in one batch): each sample is
    bit-identical to event_normalize(x[s:s+1]).  mode: int32 [S] on the device or None; a sample with mode[s] == 0 (CARRY_HOLD: no
    window this round) is not read and comes out zero-filled.  One reduce + one map launch, no host synchronisation."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise EssHipError('event_normalize_samples: x must be a CUDA(HIP) tensor; there is no CPU path')
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous() or x.numel() == 0:
        raise EssHipError(f'event_normalize_samples: x must be a non-empty contiguous fp32 [S, C, H, W] tensor, got {x.dtype}{tuple(x.shape)}')
    S = x.shape[0]
    if mode is not None:
        _stream_modes(mode, S, 'event_normalize_samples')
    if out is None:
        out = torch.empty_like(x)
    elif not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.float32 or out.shape != x.shape or not out.is_contiguous():
        raise EssHipError(f'event_normalize_samples: out must be a contiguous fp32 CUDA(HIP) tensor of x\'s shape {tuple(x.shape)}')
    ws = workspace(24 * S, x.device, 'evnorm_samples')
    _check(lib().ess_event_normalize_samples(ptr(x), ptr(out), S, x[0].numel(), ptr(mode, torch.int32), c_void_p(ws.data_ptr()), stream()),
           'ess_event_normalize_samples')
    return out


CARRY_HOLD, CARRY_TAKE, CARRY_ZERO = 0, 1, 2
STATE_CARRY_MAX_TENSORS = 16


def _carry_tensors(what, dst, src, same_streams):
    """the tensor checks of the state-carry calls -> (dst list, src list or None, streams of dst, streams of src or None).
    same_streams: src[i] has dst[i]'s whole shape (the masked call); else its per-stream shape, and all src share one stream count"""
    dst = list(dst)
    n = len(dst)
    if not 1 <= n <= STATE_CARRY_MAX_TENSORS:
        raise EssHipError(f'{what}: {n} tensors (1..{STATE_CARRY_MAX_TENSORS} per call)')
    if src is not None:
        src = list(src)
        if len(src) != n:
            raise EssHipError(f'{what}: {len(src)} source tensors for {n} destinations')
    S = S_src = None
    for i, d in enumerate(dst):
        for name, t in (('dst', d),) + ((('src', src[i]),) if src is not None else ()):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise EssHipError(f'{what}: {name}[{i}] must be a CUDA(HIP) tensor; there is no CPU path')
            if t.dim() < 1 or t.numel() == 0 or not t.is_contiguous():
                raise EssHipError(f'{what}: {name}[{i}] must be a non-empty contiguous tensor with the stream index first, got {tuple(t.shape)}')
        if src is not None and (src[i].shape[0 if same_streams else 1:] != d.shape[0 if same_streams else 1:] or src[i].dtype != d.dtype):
            raise EssHipError(f'{what}: src[{i}] is {src[i].dtype}{tuple(src[i].shape)}, dst[{i}] is {d.dtype}{tuple(d.shape)}')
        if S is None:
            S = d.shape[0]
        elif d.shape[0] != S:
            raise EssHipError(f'{what}: dst[{i}] has {d.shape[0]} streams, dst[0] has {S}')
        if src is not None:
            if S_src is None:
                S_src = src[i].shape[0]
            elif src[i].shape[0] != S_src:
                raise EssHipError(f'{what}: src[{i}] has {src[i].shape[0]} streams, src[0] has {S_src}')
        nb = d[0].numel() * d.element_size()
        if nb % 16:
            raise EssHipError(f'{what}: dst[{i}] has {nb} bytes per stream, not a multiple of 16')
    return dst, src, S, S_src


class StateCarryTable:
    """The checked host tables of one ess_state_carry_masked call, built once for a fixed set of tensors (a streaming driver's static
    state buffers and the buffers its captured step writes): dst / src lists of equally shaped tensors whose FIRST dimension is the
    stream index (any dtype: fp32 NCHW states, BF16_C8 / F16_C8 copies incl. [hi | lo], F32_C8); src None: ZERO / HOLD only.  The
    tensors are kept alive by the table."""

    def __init__(self, dst, src=None):
        dst, src, S, _ = _carry_tensors('state_carry_masked', dst, src, True)
        n = len(dst)
        self.n, self.S, self.dst, self.src = n, S, dst, src
        self.bytes_per_sample = [d[0].numel() * d.element_size() for d in dst]
        self._dst = (c_void_p * n)(*[d.data_ptr() for d in dst])
        self._src = (c_void_p * n)(*[t.data_ptr() for t in src]) if src is not None else None
        self._bytes = (c_int64 * n)(*self.bytes_per_sample)

    def run(self, mode):
        _stream_modes(mode, self.S, 'state_carry_masked')
        _check(lib().ess_state_carry_masked(self._dst, self._src, self._bytes, self.n, self.S, ptr(mode, torch.int32), stream()),
               'ess_state_carry_masked')


def state_carry_masked(dst, src, mode):
    """Per stream s (the first dimension of every tensor): mode[s] == CARRY_TAKE: dst[i][s] = src[i][s]; CARRY_ZERO: dst[i][s] = 0;
    CARRY_HOLD: dst[i][s] untouched -- for all (<= 16) tensors in ONE launch, the mode words read on the device (int32 [S]).  src
    None: no stream may TAKE.  A caller that repeats the call on the same tensors keeps a StateCarryTable and calls its run()."""
    StateCarryTable(dst, src).run(mode)


CARRY_SRC_ZERO = -1
STATE_CARRY_MAX_MOVES = 65535


class StateMoveTable:
    """The checked host tables of one ess_state_carry_indexed call, built once for a fixed set of tensors: as StateCarryTable, but dst
    and src may have DIFFERENT first dimensions (all dst share one, all src share one; src[i] has dst[i]'s dtype and per-stream
    shape) -- the home state of S streams on one side, the compact batch of a round's active streams on the other.  src None:
    zero-fills and skips only.  The tensors are kept alive by the table."""

    def __init__(self, dst, src=None):
        dst, src, S, S_src = _carry_tensors('state_carry_indexed', dst, src, False)
        n = len(dst)
        self.n, self.S_dst, self.S_src, self.dst, self.src = n, S, (S_src if src is not None else 1), dst, src
        self.bytes_per_sample = [d[0].numel() * d.element_size() for d in dst]
        self._dst = (c_void_p * n)(*[d.data_ptr() for d in dst])
        self._src = (c_void_p * n)(*[t.data_ptr() for t in src]) if src is not None else None
        self._bytes = (c_int64 * n)(*self.bytes_per_sample)

    def run(self, dst_index, src_index):
        """move p: dst record dst_index[p] = src record src_index[p] (CARRY_SRC_ZERO: = 0); a dst_index outside the destination, or
        any other src_index outside the source, skips the move.  Two contiguous int32 device tensors of equal length."""
        what = 'state_carry_indexed'
        for name, t in (('dst_index', dst_index), ('src_index', src_index)):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise EssHipError(f'{what}: {name} must be a CUDA(HIP) int32 tensor; there is no CPU path')
            if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
                raise EssHipError(f'{what}: {name} must be a contiguous int32 [n_moves] tensor, got {t.dtype}{tuple(t.shape)}')
        n_moves = dst_index.shape[0]
        if src_index.shape[0] != n_moves:
            raise EssHipError(f'{what}: {n_moves} dst_index entries for {src_index.shape[0]} src_index entries')
        if not 1 <= n_moves <= STATE_CARRY_MAX_MOVES:
            raise EssHipError(f'{what}: {n_moves} moves (1..{STATE_CARRY_MAX_MOVES} per call)')
        _check(lib().ess_state_carry_indexed(self._dst, self._src, self._bytes, self.n, self.S_dst, self.S_src, n_moves,
                                             ptr(dst_index, torch.int32), ptr(src_index, torch.int32), stream()),
               'ess_state_carry_indexed')


def state_carry_indexed(dst, src, dst_index, src_index):
    """For move p and every (<= 16) tensor i: dst[i][dst_index[p]] = src[i][src_index[p]], or = 0 where src_index[p] ==
    CARRY_SRC_ZERO; a move whose dst_index is outside dst's first dimension, or whose src_index is any other word outside src's, is
    skipped.  ONE launch, the index words read on the device (int32 [n_moves]); dst and src may have different first dimensions.
    src None: zero-fills and skips only.  A caller that repeats the call on the same tensors keeps a StateMoveTable."""
    StateMoveTable(dst, src).run(dst_index, src_index)


# ------------------------------------------------------------------------------------------ events -> voxel grids
def _slice_offsets(offsets, n_events, device):
    off = torch.as_tensor(offsets, dtype=torch.int64)
    if off.dim() != 1 or off.numel() < 2 or int(off[0]) != 0 or int(off[-1]) != n_events or bool((off[1:] < off[:-1]).any()):
        raise EssHipError('slice_offsets must be non-decreasing, start at 0 and end at the number of events')
    longest = int((off[1:] - off[:-1]).max()) if off.numel() > 1 else 0  # host-side: sizes the binning launches
    return off.to(device), longest


def voxel_grid_trilinear(x, y, pol, t, slice_offsets, channels, height, width, normalize=False, binned=True):
    """[n_slices, channels, H, W] grids of VoxelGrid.convert for every slice of a batch in one call.
    binned=False: the direct 8-atomics-per-event kernel (no workspace); default: tile-binned LDS accumulation."""
    n = x.numel()
    for a in (x, y, pol, t):
        ptr(a)
        if a.numel() != n or a.dim() != 1:
            raise EssHipError('x, y, pol, t must be 1-D and of equal length')
    off, longest = _slice_offsets(slice_offsets, n, x.device)
    ns = off.numel() - 1
    out = torch.empty(ns, channels, height, width, dtype=torch.float32, device=x.device)
    L = lib()
    wsb = L.ess_voxel_grid_trilinear_workspace(n, ns, height, width) if binned and n > 0 else 0
    ws = workspace(wsb, x.device, 'voxbin') if wsb else None
    _check(L.ess_voxel_grid_trilinear(ptr(x), ptr(y), ptr(pol), ptr(t), ptr(off, torch.int64), n, ns, channels, height, width,
                                      ptr(out), c_void_p(ws.data_ptr() if ws is not None else 0), wsb, longest, stream()),
           'ess_voxel_grid_trilinear')
    if normalize:
        voxel_normalize_(out, mode=0)
    return out


def voxel_grid_temporal(x, y, t, pol, slice_offsets, bins, height, width, separate_pol=True, normalize=False):
    """generate_voxel_grid for every slice of a batch: x, y int32 pixels, t float64, pol float32 (+1/-1, 0 = -1)."""
    n = x.numel()
    off, _ = _slice_offsets(slice_offsets, n, x.device)
    ns = off.numel() - 1
    out = torch.empty(ns, (2 if separate_pol else 1) * bins, height, width, dtype=torch.float32, device=x.device)
    _check(lib().ess_voxel_grid_temporal(ptr(x, torch.int32), ptr(y, torch.int32), ptr(t, torch.float64), ptr(pol),
                                         ptr(off, torch.int64), n, ns, bins, height, width, int(separate_pol), ptr(out), stream()),
           'ess_voxel_grid_temporal')
    if normalize:
        voxel_normalize_(out, mode=1)
    return out


# One event of the ingest path: ess_event_ingest's 16-byte record (include/ess_hip.h).  p is +1 / -1.
EVENT_RECORD = np.dtype([('t', '<f8'), ('x', '<i2'), ('y', '<i2'), ('p', '<i4')])
INGEST_KEEP = -1  # ESS_INGEST_KEEP: a count word that leaves the stream's grid in `out` as it is
INGEST_MAX_CAPACITY = 1 << 22


def _are_tensors(fn, named):
    for name, v in named:
        if not torch.is_tensor(v):
            raise EssHipError(f'{fn}: {name} must be a CUDA(HIP) tensor; there is no CPU path')


def _on_device(fn, named):
    """the last check of a binding: what is wrong with a tensor's form is said whatever memory it lies in"""
    for name, v in named:
        if not v.is_cuda:
            raise EssHipError(f'{fn}: {name} must be a CUDA(HIP) tensor; there is no CPU path')
        if not v.is_contiguous():
            raise EssHipError(f'{fn}: {name} must be contiguous')


def _ingest_out(fn, out, n_name):
    """the grids an ingest fills -> (n, bins, H, W)"""
    if out.dim() != 4 or out.dtype != torch.float32 or out.numel() == 0:
        raise EssHipError(f'{fn}: out must be a non-empty fp32 [{n_name}, bins, H, W] tensor, got {out.dtype}{tuple(out.shape)}')
    return out.shape


def _ingest_acc(fn, named, acc, out):
    """the last checks of an ingest binding -- acc's dtype, then _on_device -- and the all-zero sums of a call that gave none"""
    if acc is not None and acc.dtype != torch.int64:
        raise EssHipError(f'{fn}: acc must be int64, got {acc.dtype}')
    _on_device(fn, named)
    if acc is None:
        acc = torch.zeros(out.numel(), dtype=torch.int64, device=out.device)
    return acc


def event_ingest(records, counts, out, acc=None):
    """Packed event records -> one signed temporal voxel grid per stream, ORDER-INDEPENDENT: each contribution is the fp32 value
    voxel_grid_temporal(separate_pol=False) adds, summed as a 64-bit integer at scale 2^40, so out is a pure function of the set of
    events (bit-identical run to run, batched or alone, whatever the record order between the first and the last).
    records: device uint8 [S, capacity, 16] (EVENT_RECORD rows; datasets.data_util.pack_event_records fills them on the host);
    counts: device int32 [S], read on the device -- n > 0: the stream's first n records, 0: an all-zero grid, INGEST_KEEP (< 0):
    out[s] is neither read nor written; out: fp32 [S, bins, H, W], returned.  acc: a contiguous device int64 tensor of at least
    S * bins * H * W elements that is ALL ZERO (it is again behind the call) or None: allocated and zeroed here.  Two launches
    whose shape follows from the capacity alone, no memset and no synchronisation: capturable as they stand."""
    for name, t in (('records', records), ('counts', counts), ('out', out)) + ((('acc', acc),) if acc is not None else ()):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise EssHipError(f'event_ingest: {name} must be a CUDA(HIP) tensor; there is no CPU path')
        if not t.is_contiguous():
            raise EssHipError(f'event_ingest: {name} must be contiguous')
    if out.dim() != 4 or out.dtype != torch.float32 or out.numel() == 0:
        raise EssHipError(f'event_ingest: out must be a non-empty fp32 [S, bins, H, W] tensor, got {out.dtype}{tuple(out.shape)}')
    S, bins, H, W = out.shape
    if records.dtype != torch.uint8 or records.dim() != 3 or records.shape[0] != S or records.shape[2] != EVENT_RECORD.itemsize or records.shape[1] < 1:
        raise EssHipError(f'event_ingest: records must be uint8 [{S}, capacity, {EVENT_RECORD.itemsize}], got {records.dtype}{tuple(records.shape)}')
    if counts.dtype != torch.int32 or tuple(counts.shape) != (S,):
        raise EssHipError(f'event_ingest: counts must be int32 [{S}], got {counts.dtype}{tuple(counts.shape)}')
    L = lib()
    need = L.ess_event_ingest_workspace(S, bins, H, W)
    if acc is None:
        acc = torch.zeros(need // 8, dtype=torch.int64, device=out.device)
    elif acc.dtype != torch.int64:
        raise EssHipError(f'event_ingest: acc must be int64, got {acc.dtype}')
    _check(L.ess_event_ingest(c_void_p(records.data_ptr()), ptr(counts, torch.int32), records.shape[1], S, bins, H, W,
                              c_void_p(acc.data_ptr()), acc.numel() * 8, c_void_p(out.data_ptr()), stream()), 'ess_event_ingest')
    return out


# The column source of the ingest (ess_event_ingest_columns): the per-stream format word's bits, and the row stride of a capacity
EVCOL_T_I64 = 1   # ESS_EVCOL_T_I64: t is int64 (else float64)
EVCOL_XY_U16 = 2  # ESS_EVCOL_XY_U16: x / y are uint16 (else int16)
EVCOL_STRIDE_ALIGN = 16


def event_column_stride(capacity):
    """events per stream -> the row stride of the column buffers: rounded up so that every stream's row of every column (the
    1-byte polarities too) starts 16-byte aligned"""
    return -(-int(capacity) // EVCOL_STRIDE_ALIGN) * EVCOL_STRIDE_ALIGN


_EVCOL_DTYPES = {'t': (torch.int64, torch.float64), 'x': (torch.int16,) + ((torch.uint16,) if hasattr(torch, 'uint16') else ()),
                 'p': (torch.uint8, torch.int8, torch.bool)}
_EVCOL_DTYPES['y'] = _EVCOL_DTYPES['x']


def event_ingest_columns(t, x, y, p, counts, formats, out, acc=None):
    """event_ingest from raw event columns: the same grids, bit for bit, as event_ingest gives on the same events.
    t, x, y, p: device [S, stride] -- t 8 bytes per event (int64 or float64), x / y 2 bytes (int16 or uint16), p 1 byte (uint8, int8
    or bool); the tensors' dtypes only size the words: how stream s's words are READ says formats[s] (EVCOL_T_I64 | EVCOL_XY_U16; any
    other bit: the stream counts as empty), a device int32 [S] read by the kernel like counts, so one captured call serves streams
    whose formats change from round to round.  p: +1 where the byte equals 1, -1 otherwise.  stride: a multiple of 16
    (event_column_stride).  counts, out, acc: as event_ingest."""
    return _event_call('event_ingest_columns', 'columns', 'plain', (t, x, y, p), (counts, formats), out, acc, 'required')


def _event_columns(fn, named, n, ring):
    """The tensors a column-source call reads.  named[:4]: the raw columns t, x, y, p -- [n, stride] each, or (ring) [n_rows, ring]
    with ring a multiple of 16 inside the capacity (a stride is the library's to check); named[4:]: the device words, int32 [n]."""
    t = named[0][1]
    if t.dim() != 2 or t.shape[1] < 1 or (t.shape[0] < 1 if ring else t.shape[0] != n):
        form = 'n_rows, ring' if ring else f'{n}, stride'
        raise EssHipError(f'{fn}: t must be [{form}], got {tuple(t.shape)}')
    for name, v in named[:4]:
        if v.dtype not in _EVCOL_DTYPES[name] or v.shape != t.shape:
            raise EssHipError(f'{fn}: {name} must be {" / ".join(str(d) for d in _EVCOL_DTYPES[name])} '
                              f'{list(t.shape)}, got {v.dtype}{tuple(v.shape)}')
    for name, v in named[4:]:
        if v.dtype != torch.int32 or tuple(v.shape) != (n,):
            raise EssHipError(f'{fn}: {name} must be int32 [{n}], got {v.dtype}{tuple(v.shape)}')
    if ring and (t.shape[1] % EVCOL_STRIDE_ALIGN or t.shape[1] > INGEST_MAX_CAPACITY):
        raise EssHipError(f'{fn}: ring={t.shape[1]} must be a multiple of {EVCOL_STRIDE_ALIGN} in [{EVCOL_STRIDE_ALIGN}, '
                          f'{INGEST_MAX_CAPACITY}] (event_column_stride rounds a capacity up)')


def _column_pointers(named):
    """t, x, y, p as untyped pointers, the int32 words behind them"""
    return [c_void_p(v.data_ptr()) for _, v in named[:4]] + [ptr(v, torch.int32) for _, v in named[4:]]


_EVENT_WORDS = {'columns': ('counts', 'formats'), 'ring': ('rows', 'starts', 'counts', 'formats'), 'store': ('starts', 'counts', 'formats')}
_NO_RECTIFY = (c_void_p(0), c_void_p(0), 0, 1, 1)


def _event_call(fn, kind, form, cols, words, out, acc, has_out, representation=None, trilinear=False, rectify=(None, None),
                masks=(None, None, None), flavour=None, total=None, window_capacity=None):
    """The one body behind the column / ring / store bindings: the checks in their order -- what is wrong with a tensor's form is said
    whatever memory it lies in, acc's dtype, the device and contiguity last -- and the call of ess_<fn>.
    kind: 'columns', 'ring' or 'store', the source: cols = (t, x, y, p), words = its device words (_EVENT_WORDS names them).
    form: what the entry point takes behind the grids -- 'plain' nothing, 'trilinear' the rectify arguments, 'rep' a representation
    word, 'masked' representation, trilinear, rectify and mask arguments, 'store' / 'store_masked' a flavour word, rectify (and
    mask) arguments.  has_out: 'required', 'optional' (None: scatter only, acc keeps the sums and is returned) or 'none' (the
    entry point has no out).  -> out, or acc where there is no out"""
    cols, words = tuple(zip('txyp', cols)), tuple(zip(_EVENT_WORDS[kind], words))
    if has_out == 'optional' and out is None and acc is None:
        raise EssHipError(f'{fn}: out=None (scatter only) needs acc, the int64 [n_slots, C, H, W] sums it leaves')
    named = cols + words + ((('out', out),) if out is not None or has_out == 'required' else ()) + \
        ((('acc', acc),) if acc is not None or has_out == 'none' else ())
    _are_tensors(fn, named)
    where = 'out' if out is not None else 'acc'
    n_name = 'S' if kind == 'columns' and form != 'masked' else 'n_slots'
    n, C, H, W = _ingest_out(fn, out, n_name) if out is not None else _finish_acc(fn, acc, 'H, W')
    maps, map_of = rectify
    tail = ()
    if kind == 'store':
        if isinstance(flavour, bool) or flavour not in _EVENT_STORE_FLAVOURS:
            raise EssHipError(f'{fn}: flavour={flavour!r} must be EVENT_STORE_SIGNED, _SEPARATE, _HISTOGRAM or _TRILINEAR')
        trilinear = flavour == EVENT_STORE_TRILINEAR
        if not trilinear:
            _event_rep_of(fn, int(flavour), C, where)
            if maps is not None or map_of is not None:
                raise EssHipError(f'{fn}: maps / map_of belong to flavour=EVENT_STORE_TRILINEAR')
        tail = (int(flavour),)
    elif form in ('rep', 'masked'):
        rep = _event_rep_of(fn, representation, C, where)
        tail = (rep,)
    if form == 'masked':
        if not isinstance(trilinear, (bool, int)) or trilinear not in (0, 1):
            raise EssHipError(f'{fn}: trilinear={trilinear!r} must be False or True')
        if trilinear and rep != EVENT_REP_SIGNED:
            raise EssHipError(f'{fn}: trilinear=True builds the signed grid alone, representation={representation!r} must be EVENT_REP_SIGNED')
        if not trilinear and (maps is not None or map_of is not None):
            raise EssHipError(f'{fn}: maps / map_of are read by the trilinear flavour alone (trilinear=False)')
        tail += (int(trilinear),)
    t = cols[0][1]
    if kind == 'store':
        capacity, total = _store_columns(fn, cols, total)
        window_capacity = _int_in(fn, 'window_capacity', window_capacity, 1, INGEST_MAX_CAPACITY)
        _formed_words(fn, words[:1], torch.int64, (n,))
        _formed_words(fn, words[1:], torch.int32, (n,))
    else:
        _event_columns(fn, cols + words, n, ring=kind == 'ring')
    takes_masks = form in ('masked', 'store_masked')
    mask_form = _mask_form(fn, *masks, n) if takes_masks else None
    if out is not None:
        acc = _ingest_acc(fn, named, acc, out)
    else:
        _on_device(fn, named)
    if form not in ('plain', 'rep'):
        tail += _rectify_args(fn, maps, map_of, n, acc.device) if trilinear or form == 'trilinear' else _NO_RECTIFY
    if takes_masks:
        tail += _mask_args(fn, masks[0], masks[1], mask_form, n, acc.device)
    if kind == 'store':
        source = [c_void_p(v.data_ptr()) for _, v in cols] + [ptr(words[0][1], torch.int64)] + [ptr(v, torch.int32) for _, v in words[1:]] + \
            [capacity, total, window_capacity]
    else:
        source = _column_pointers(cols + words)
        if form == 'masked' and kind == 'columns':  # (the one entry point of both sources: no rows, no starts)
            source[4:4] = [c_void_p(0), c_void_p(0)]
        source += [t.shape[1]] + ([t.shape[0]] if kind == 'ring' or form == 'masked' else [])
    out_arg = () if has_out == 'none' else (c_void_p(0 if out is None else out.data_ptr()),)
    _check(getattr(lib(), 'ess_' + fn)(*source, n, C, H, W, c_void_p(acc.data_ptr()), acc.numel() * 8, *out_arg, *tail, stream()), 'ess_' + fn)
    return out if out is not None else acc


RECTIFY_NONE = -1  # ESS_RECTIFY_NONE: a map word for a stream whose raw pixels are its coordinates
RECTIFY_MAX_SIDE = 32768


def _rectify_args(fn, maps, map_of, n, device):
    """maps: None or device fp32 [n_maps, map_h, map_w, 2]; map_of: None (RECTIFY_NONE for every slot) or device int32 [n] -> the
    five rectify arguments of the trilinear entry points.  Without maps the map size is (1, 1): no word names a map."""
    if maps is None:
        n_maps, mh, mw = 0, 1, 1
    else:
        if not torch.is_tensor(maps) or maps.dtype != torch.float32 or maps.dim() != 4 or maps.shape[3] != 2 or maps.numel() == 0:
            got = f'{maps.dtype}{tuple(maps.shape)}' if torch.is_tensor(maps) else type(maps).__name__
            raise EssHipError(f'{fn}: maps must be a non-empty fp32 [n_maps, map_h, map_w, 2] tensor or None, got {got}')
        n_maps, mh, mw = maps.shape[:3]
        if mh > RECTIFY_MAX_SIDE or mw > RECTIFY_MAX_SIDE:
            raise EssHipError(f'{fn}: maps of {mh} x {mw} pixels: a side is 1..{RECTIFY_MAX_SIDE}')
    if map_of is None:
        map_of = torch.full((n,), RECTIFY_NONE, dtype=torch.int32, device=device)
    elif not torch.is_tensor(map_of) or map_of.dtype != torch.int32 or tuple(map_of.shape) != (n,):
        got = f'{map_of.dtype}{tuple(map_of.shape)}' if torch.is_tensor(map_of) else type(map_of).__name__
        raise EssHipError(f'{fn}: map_of must be int32 [{n}] or None, got {got}')
    for name, v in (('maps', maps), ('map_of', map_of)):
        if v is not None and not v.is_cuda:
            raise EssHipError(f'{fn}: {name} must be a CUDA(HIP) tensor; there is no CPU path')
        if v is not None and not v.is_contiguous():
            raise EssHipError(f'{fn}: {name} must be contiguous')
    return (c_void_p(0 if maps is None else maps.data_ptr()), ptr(map_of, torch.int32), n_maps, mh, mw)


def event_ingest_columns_trilinear(t, x, y, p, counts, formats, out, maps=None, map_of=None, acc=None):
    """event_ingest_columns in the TRILINEAR flavour, the grid the DSEC loader builds: each raw (x, y) goes through its stream's
    rectify map, the float coordinates and the time -- normalised in fp32 as the loader does -- are spread over the up to eight
    corners VoxelGrid.convert gives them (hip.voxel_grid_trilinear's per-event expressions), and the contributions are summed in
    64-bit fixed point like the temporal flavour's: out is a pure function of the set of events.  maps: device fp32
    [n_maps, map_h, map_w, 2], entry [y, x] = the rectified (x, y) -- the SENSOR's size, whatever the grid's -- or None; map_of:
    device int32 [S], read on the device -- RECTIFY_NONE: the integer pixel is the coordinate, 0 .. n_maps - 1: that map (a raw
    pixel outside it drops the event), anything else: the stream counts as empty -- or None: RECTIFY_NONE throughout.  A window
    whose last time equals its first gives an all-zero grid.  VoxelGrid(normalize=True)'s own normalisation is not applied.
    Everything else: as event_ingest_columns."""
    return _event_call('event_ingest_columns_trilinear', 'columns', 'trilinear', (t, x, y, p), (counts, formats), out, acc, 'required',
                       rectify=(maps, map_of))


def event_ingest_ring(t, x, y, p, rows, starts, counts, formats, out, acc=None):
    """event_ingest_columns on windows named inside per-stream event RINGS: the same grids, bit for bit, as event_ingest_columns
    gives on the same windows laid out from entry 0.  t, x, y, p: device [n_rows, ring] raw columns (dtypes as event_ingest_columns),
    row r the ring stream r's packets are appended to; ring: a multiple of 16.  rows, starts, counts, formats: device int32
    [n_slots], all read on the device -- slot i's window is the counts[i] events of row rows[i] at (starts[i] + k) mod ring; count 0:
    an all-zero grid, INGEST_KEEP (< 0): out[i] is neither read nor written, a count above ring: ring; a row outside [0, n_rows), a
    start outside [0, ring) or an unknown format bit: the slot counts as empty.  Two slots may name one row.  out: fp32
    [n_slots, bins, H, W], returned; acc: as event_ingest, at least n_slots * bins * H * W elements."""
    return _event_call('event_ingest_ring', 'ring', 'plain', (t, x, y, p), (rows, starts, counts, formats), out, acc, 'required')


def event_ingest_ring_trilinear(t, x, y, p, rows, starts, counts, formats, out, maps=None, map_of=None, acc=None):
    """event_ingest_ring in the trilinear flavour: the same grids, bit for bit, as event_ingest_columns_trilinear gives on the same
    windows laid out from entry 0.  maps, map_of (int32 [n_slots], slot i's map): as event_ingest_columns_trilinear; everything else:
    as event_ingest_ring."""
    return _event_call('event_ingest_ring_trilinear', 'ring', 'trilinear', (t, x, y, p), (rows, starts, counts, formats), out, acc,
                       'required', rectify=(maps, map_of))


# The ring ingest in its two halves (ess_event_scatter_ring* / ess_event_grid_finish): the LOADER's grid -- normalised over its
# non-zero voxels, rows cut, resized bilinearly -- from the same order-independent sums.
GRID_NORM_NONE = 0        # ESS_GRID_NORM_NONE
GRID_NORM_UNBIASED = 1    # ESS_GRID_NORM_UNBIASED: VoxelGrid(normalize=True)
GRID_NORM_POPULATION = 2  # ESS_GRID_NORM_POPULATION: normalize_voxel_grid


def event_scatter_ring(t, x, y, p, rows, starts, counts, formats, acc):
    """The first half of event_ingest_ring: the windows' events are added into acc and nothing else happens.  acc: device int64
    [n_slots, bins, H, W] -- the grid's geometry is read from it -- ALL ZERO before the call; behind it it holds the sums at scale 2^40
    that event_grid_finish turns into grids (and zeroes again).  t .. formats: as event_ingest_ring.  -> acc"""
    return _event_call('event_scatter_ring', 'ring', 'plain', (t, x, y, p), (rows, starts, counts, formats), None, acc, 'none')


def event_scatter_ring_trilinear(t, x, y, p, rows, starts, counts, formats, acc, maps=None, map_of=None):
    """event_scatter_ring in the trilinear flavour: the first half of event_ingest_ring_trilinear; maps, map_of: as there."""
    return _event_call('event_scatter_ring_trilinear', 'ring', 'trilinear', (t, x, y, p), (rows, starts, counts, formats), None, acc,
                       'none', rectify=(maps, map_of))


# The event REPRESENTATIONS of the column / ring ingest (ess_event_*_rep): what the reference's loaders hand the network
# (datasets/data_util.py:6-126 there, `event_representation` and `separate_pol` in its settings).
EVENT_REP_SIGNED = 0     # ESS_EVENT_REP_SIGNED: the signed temporal voxel grid, `bins` planes (event_ingest_columns' own grid)
EVENT_REP_SEPARATE = 1   # ESS_EVENT_REP_SEPARATE: 2 * bins planes [positive bins; negative bins], both halves non-negative
EVENT_REP_HISTOGRAM = 2  # ESS_EVENT_REP_HISTOGRAM: 2 planes [negative counts, positive counts]; the time column is not read
_EVENT_REPS = (EVENT_REP_SIGNED, EVENT_REP_SEPARATE, EVENT_REP_HISTOGRAM)


def _event_rep(fn, representation):
    if isinstance(representation, bool) or not isinstance(representation, int) or representation not in _EVENT_REPS:
        raise EssHipError(f'{fn}: representation={representation!r} must be EVENT_REP_SIGNED, EVENT_REP_SEPARATE or EVENT_REP_HISTOGRAM')
    return representation


def event_rep_channels(representation, bins):
    """the planes C of one grid: bins (EVENT_REP_SIGNED), 2 * bins (EVENT_REP_SEPARATE), 2 whatever bins is (EVENT_REP_HISTOGRAM)"""
    rep = _event_rep('event_rep_channels', representation)
    if isinstance(bins, bool) or not isinstance(bins, int) or bins < 1:
        raise EssHipError(f'event_rep_channels: bins={bins!r} must be a positive int')
    return (bins, 2 * bins, 2)[rep]


def _event_rep_of(fn, representation, channels, where):
    """the representation word, checked against the planes of the grid it fills (`where` names the tensor they were read from)"""
    rep = _event_rep(fn, representation)
    if rep == EVENT_REP_SEPARATE and channels % 2:
        raise EssHipError(f'{fn}: representation=EVENT_REP_SEPARATE fills 2 * bins planes [positive; negative], {where} has channels={channels}')
    if rep == EVENT_REP_HISTOGRAM and channels != 2:
        raise EssHipError(f'{fn}: representation=EVENT_REP_HISTOGRAM fills 2 planes [negative, positive], {where} has channels={channels}')
    return rep


EVENT_REPRESENTATIONS = {None: EVENT_REP_SIGNED, 'separate_pol': EVENT_REP_SEPARATE, 'histogram': EVENT_REP_HISTOGRAM}


def event_representation(representation, voxel, rectify_maps):
    """The representation= keyword of EventBatchBuilder and the segmenters, checked against their voxel= and rectify_maps= -> the
    EVENT_REP_* word.  None: the signed grid, whatever the flavour.  'separate_pol' / 'histogram' are built by the temporal
    loader on integer pixels: the reference's DSEC voxel_grid path ignores separate_pol too, and a rectified histogram is no grid
    the reference builds."""
    if not isinstance(representation, (str, type(None))) or representation not in EVENT_REPRESENTATIONS:
        raise EssHipError(f"representation={representation!r}: None (the signed grid), 'separate_pol' or 'histogram'")
    if representation is not None and (voxel != 'temporal' or rectify_maps is not None):
        raise EssHipError(f"representation={representation!r} is built from integer pixels by the temporal loader: it needs "
                          f"voxel='temporal' and rectify_maps=None (got voxel={voxel!r}, rectify_maps "
                          f"{'given' if rectify_maps is not None else 'None'})")
    return EVENT_REPRESENTATIONS[representation]


def event_scatter_ring_rep(t, x, y, p, rows, starts, counts, formats, acc, representation):
    """event_scatter_ring in one of the three event representations.  acc: device int64 [n_slots, C, H, W], ALL ZERO before the
    call; representation (a host int, fixed per call):
        EVENT_REP_SIGNED:    C = bins; event_scatter_ring's own sums, bit for bit;
        EVENT_REP_SEPARATE:  C = 2 * bins (even).  Window, validity test, bin and the two weights left = fp32(1 - dts), right =
                             fp32(dts) are event_scatter_ring's; NO sign is applied (the reference adds |pol| * weight): a positive
                             event (byte == 1) adds to planes ti and ti + 1, any other to planes bins + ti and bins + ti + 1, the
                             right half dropped where ti + 1 == bins.  sums[b] - sums[bins + b] is the signed grid's sum, exactly;
        EVENT_REP_HISTOGRAM: C = 2.  Plane 0 counts the events of pixel (x, y) whose polarity byte is not 1, plane 1 those whose
                             byte is 1, 2^40 each.  The time column is NOT READ (t still gives the rings' shape): an event counts
                             whatever its time is, a NaN included.  Coordinates outside [0, W) x [0, H) are DROPPED; the reference
                             neither checks nor drops them (x + width * y wraps into a neighbouring row, or raises): not reproduced.
    Counts, rows, starts, format words and INGEST_KEEP: as event_ingest_ring.  The sums stay a pure function of the SET of events;
    event_grid_finish* turn them into grids over all C planes of a slot.  -> acc"""
    return _event_call('event_scatter_ring_rep', 'ring', 'rep', (t, x, y, p), (rows, starts, counts, formats), None, acc, 'none',
                       representation=representation)


def event_ingest_ring_rep(t, x, y, p, rows, starts, counts, formats, out, representation, acc=None):
    """event_ingest_ring in one of the three event representations (event_scatter_ring_rep names them): the scatter and the plain
    finish, out fp32 [n_slots, C, H, W] = (float)sums * 2^-40, returned.  EVENT_REP_SIGNED gives event_ingest_ring's bits.
    Everything else: as event_ingest_ring; acc: at least n_slots * C * H * W elements."""
    return _event_call('event_ingest_ring_rep', 'ring', 'rep', (t, x, y, p), (rows, starts, counts, formats), out, acc, 'required',
                       representation=representation)


def event_ingest_columns_rep(t, x, y, p, counts, formats, out, representation, acc=None):
    """event_ingest_columns in one of the three event representations (event_scatter_ring_rep names them): out fp32 [S, C, H, W],
    returned.  EVENT_REP_SIGNED gives event_ingest_columns' bits.  Everything else: as event_ingest_columns."""
    return _event_call('event_ingest_columns_rep', 'columns', 'rep', (t, x, y, p), (counts, formats), out, acc, 'required',
                       representation=representation)


# Hot-pixel masks (ess_event_ingest_masked / ess_event_hot_pixel_mask): per-sensor bit masks applied to the RAW events
MASK_NONE = -1     # ESS_MASK_NONE: a mask word for a slot without a mask
MASK_REPLACE = 0   # ESS_MASK_REPLACE: event_hot_pixel_mask writes whole words, the tail bits of a row as 0
MASK_OR = 1        # ESS_MASK_OR: ... or-s the new bits onto the words that are there
MASK_MAX_SIDE = 32768
_MASK_DTYPES = (torch.int32,) + ((torch.uint32,) if hasattr(torch, 'uint32') else ())


def mask_words(width):
    """32-bit words in one row of a hot-pixel mask of `width` pixels"""
    return (int(width) + 31) // 32


def _mask_tensor(fn, masks, size, lead):
    """masks: device int32 / uint32 [n, h, ceil(w / 32)] with size = (h, w) -> (n, h, w); what is wrong with its form is said here"""
    if not isinstance(size, (tuple, list)) or len(size) != 2 or \
            any(isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= MASK_MAX_SIDE for v in size):
        raise EssHipError(f'{fn}: mask_size={size!r} must be (mask_h, mask_w), the sensor\'s size, 1..{MASK_MAX_SIDE} each')
    h, w = size
    if not torch.is_tensor(masks) or masks.dtype not in _MASK_DTYPES or masks.dim() != 3 or masks.numel() == 0 \
            or tuple(masks.shape[1:]) != (h, mask_words(w)):
        got = f'{masks.dtype}{tuple(masks.shape)}' if torch.is_tensor(masks) else type(masks).__name__
        raise EssHipError(f'{fn}: masks must be a non-empty int32 / uint32 [{lead}, {h}, {mask_words(w)}] tensor '
                          f'(bit x & 31 of word x >> 5 of row y: pixel (x, y) of a {h} x {w} sensor), got {got}')
    return masks.shape[0], h, w


def _mask_form(fn, masks, mask_of, mask_size, n):
    """the form of masks (None or int32 / uint32 [n_masks, mask_h, ceil(mask_w / 32)] with mask_size = (mask_h, mask_w)) and of mask_of
    (None or int32 [n]), whatever memory they lie in -> (n_masks, mask_h, mask_w)"""
    if masks is None:
        if mask_size is not None:
            raise EssHipError(f'{fn}: mask_size={mask_size!r} without masks')
        n_masks, mh, mw = 0, 1, 1
    else:
        n_masks, mh, mw = _mask_tensor(fn, masks, mask_size, 'n_masks')
    if mask_of is not None and (not torch.is_tensor(mask_of) or mask_of.dtype != torch.int32 or tuple(mask_of.shape) != (n,)):
        got = f'{mask_of.dtype}{tuple(mask_of.shape)}' if torch.is_tensor(mask_of) else type(mask_of).__name__
        raise EssHipError(f'{fn}: mask_of must be int32 [{n}] or None, got {got}')
    return n_masks, mh, mw


def _mask_args(fn, masks, mask_of, form, n, device):
    """the checked masks / mask_of (None: MASK_NONE for every slot) and _mask_form's answer -> the five mask arguments of
    event_ingest_masked"""
    n_masks, mh, mw = form
    if mask_of is None:
        mask_of = torch.full((n,), MASK_NONE, dtype=torch.int32, device=device)
    for name, v in (('masks', masks), ('mask_of', mask_of)):
        if v is not None and not v.is_cuda:
            raise EssHipError(f'{fn}: {name} must be a CUDA(HIP) tensor; there is no CPU path')
        if v is not None and not v.is_contiguous():
            raise EssHipError(f'{fn}: {name} must be contiguous')
    return (c_void_p(0 if masks is None else masks.data_ptr()), ptr(mask_of, torch.int32), n_masks, mh, mw)


def event_ingest_masked(t, x, y, p, rows, starts, counts, formats, out, masks=None, mask_of=None, mask_size=None,
                        representation=EVENT_REP_SIGNED, trilinear=False, maps=None, map_of=None, acc=None):
    """The column / ring ingest behind per-sensor HOT-PIXEL MASKS, applied to the raw events: one call for both sources, every
    flavour and both halves.  rows, starts: device int32 [n_slots] (the ring source, t .. p [n_rows, ring]) or both None (the column
    source, t .. p [n_slots, stride], slot s's window at the head of row s).  out: fp32 [n_slots, C, H, W], returned -- or None:
    scatter only, acc (then required: int64 [n_slots, C, H, W], all zero before) keeps the sums for event_grid_finish*, and is
    returned.  representation: EVENT_REP_*; trilinear=True: the trilinear flavour with maps / map_of as
    event_ingest_ring_trilinear takes them (representation must be EVENT_REP_SIGNED).
    masks: device int32 / uint32 [n_masks, mask_h, ceil(mask_w / 32)], pixel (x, y) = bit x & 31 of word x >> 5 of row y, set: hot
    (datasets.hot_pixels.HotPixelMask.words), with mask_size=(mask_h, mask_w) the SENSOR's size whatever the grid's -- or None;
    mask_of: device int32 [n_slots], read on the device -- MASK_NONE: no mask, 0 .. n_masks - 1: that mask, anything else: the slot
    counts as empty -- or None: MASK_NONE throughout.  An event whose raw (x, y) lies inside the mask with its bit set is dropped
    BEFORE the flavour sees it (before a rectify map moves it); every other event is handled as the unmasked entry points handle
    it.  The window's time base comes from its first and last event whether they are masked or not (the reference voxelises
    first and zeroes afterwards).  Everything else: as event_ingest_ring_rep / event_ingest_columns_rep."""
    fn = 'event_ingest_masked'
    if (rows is None) != (starts is None):
        raise EssHipError(f'{fn}: rows and starts are both given (the ring source) or both None (the column source)')
    kind, words = ('columns', (counts, formats)) if rows is None else ('ring', (rows, starts, counts, formats))
    return _event_call(fn, kind, 'masked', (t, x, y, p), words, out, acc, 'optional', representation=representation, trilinear=trilinear,
                       rectify=(maps, map_of), masks=(masks, mask_of, mask_size))


def event_hot_pixel_mask(sums, thresholds, masks, mode=MASK_REPLACE):
    """Per-pixel event counts -> hot-pixel masks.  sums: device int64 [n, 2, H, W], what event_scatter_ring_rep(EVENT_REP_HISTOGRAM)
    leaves (2^40 per event; read only -- the sums of several scatters onto one acc may be thresholded, as long as no pixel
    collects more than 2^22 events).  thresholds: device int64 [n], in EVENTS, read on the device: >= 0 -- bit (y, x) of masks[i] is
    set iff the pixel's events of both polarities together number MORE than thresholds[i]; < 0 -- masks[i] is neither read nor
    written.  masks: device int32 / uint32 [n, H, ceil(W / 32)] (the layout event_ingest_masked reads), returned.  mode:
    MASK_REPLACE -- whole words are written, the bits at x >= W of a row's last word as 0; MASK_OR -- the new bits are or-ed onto what
    is there, the tail bits stay.  One launch shaped by the sizes alone, no atomics, no memset: capturable."""
    fn = 'event_hot_pixel_mask'
    named = (('sums', sums), ('thresholds', thresholds), ('masks', masks))
    _are_tensors(fn, named)
    if sums.dim() != 4 or sums.dtype != torch.int64 or sums.numel() == 0 or sums.shape[1] != 2:
        raise EssHipError(f'{fn}: sums must be a non-empty int64 [n, 2, H, W] tensor (the histogram flavour\'s sums), '
                          f'got {sums.dtype}{tuple(sums.shape)}')
    n, _, H, W = sums.shape
    if H > MASK_MAX_SIDE or W > MASK_MAX_SIDE:
        raise EssHipError(f'{fn}: sums of {H} x {W} pixels: a side is 1..{MASK_MAX_SIDE}')
    if thresholds.dtype != torch.int64 or tuple(thresholds.shape) != (n,):
        raise EssHipError(f'{fn}: thresholds must be int64 [{n}], got {thresholds.dtype}{tuple(thresholds.shape)}')
    if _mask_tensor(fn, masks, (H, W), n)[0] != n:
        raise EssHipError(f'{fn}: masks must hold {n} masks, one per sensor of sums, got {tuple(masks.shape)}')
    if isinstance(mode, bool) or mode not in (MASK_REPLACE, MASK_OR):
        raise EssHipError(f'{fn}: mode={mode!r} must be MASK_REPLACE or MASK_OR')
    _on_device(fn, named)
    _check(lib().ess_event_hot_pixel_mask(c_void_p(sums.data_ptr()), n, H, W, c_void_p(thresholds.data_ptr()), c_void_p(masks.data_ptr()),
                                          int(mode), stream()), 'ess_' + fn)
    return masks


def _finish_acc(fn, acc, dims):
    """the sums a scatter leaves and a loader finish reads -> (n_slots, bins, Hs, Ws)"""
    if acc.dim() != 4 or acc.dtype != torch.int64 or acc.numel() == 0:
        raise EssHipError(f'{fn}: acc must be a non-empty int64 [n_slots, bins, {dims}] tensor, got {acc.dtype}{tuple(acc.shape)}')
    return acc.shape


# The device event store (ess_event_scatter_store / ess_event_store_windows): windows cut on the device out of recordings that were
# uploaded once (datasets.event_store.EventStore owns the columns and the recording table).
EVENT_STORE_SIGNED = 0      # ESS_EVENT_STORE_SIGNED: EVENT_REP_SIGNED's grid
EVENT_STORE_SEPARATE = 1    # ESS_EVENT_STORE_SEPARATE: EVENT_REP_SEPARATE's
EVENT_STORE_HISTOGRAM = 2   # ESS_EVENT_STORE_HISTOGRAM: EVENT_REP_HISTOGRAM's
EVENT_STORE_TRILINEAR = 3   # ESS_EVENT_STORE_TRILINEAR: event_scatter_ring_trilinear's grid, with maps / map_of
EVENT_STORE_RULE_COUNT_TIME = 0   # ESS_EVENT_STORE_RULE_COUNT_TIME: T * n events before the first event with t >= bound
EVENT_STORE_RULE_COUNT_INDEX = 1  # ESS_EVENT_STORE_RULE_COUNT_INDEX: ... before the given index of the recording
EVENT_STORE_RULE_DURATION = 2     # ESS_EVENT_STORE_RULE_DURATION: T windows between T + 1 time bounds
EVENT_STORE_FLAG_EMPTY = 1     # ESS_EVENT_STORE_FLAG_EMPTY: no event in any window of the sample
EVENT_STORE_FLAG_OVERFLOW = 2  # ESS_EVENT_STORE_FLAG_OVERFLOW: a window above window_capacity; all T counts are 0
EVENT_STORE_FLAG_RANGE = 4     # ESS_EVENT_STORE_FLAG_RANGE: the recording or the end index lies outside the table / the recording
EVENT_STORE_MAX_CAPACITY = 1 << 40
EVENT_STORE_TABLE_WORDS = 4    # a recording's row: begin, end, format, reserved
_EVENT_STORE_FLAVOURS = (EVENT_STORE_SIGNED, EVENT_STORE_SEPARATE, EVENT_STORE_HISTOGRAM, EVENT_STORE_TRILINEAR)
_EVENT_STORE_RULES = (EVENT_STORE_RULE_COUNT_TIME, EVENT_STORE_RULE_COUNT_INDEX, EVENT_STORE_RULE_DURATION)


def _int_in(fn, name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise EssHipError(f'{fn}: {name}={v!r} must be an int in [{lo}, {hi}]')
    return int(v)


def _store_columns(fn, named, total):
    """the store's flat columns t, x, y, p [capacity] -> (capacity, total)"""
    t = named[0][1]
    if t.dim() != 1 or t.shape[0] < EVCOL_STRIDE_ALIGN or t.shape[0] % EVCOL_STRIDE_ALIGN or t.shape[0] > EVENT_STORE_MAX_CAPACITY:
        raise EssHipError(f'{fn}: t must be [capacity], capacity a multiple of {EVCOL_STRIDE_ALIGN} in [{EVCOL_STRIDE_ALIGN}, 2^40], '
                          f'got {tuple(t.shape)}')
    for name, v in named[:4]:
        if v.dtype not in _EVCOL_DTYPES[name] or v.shape != t.shape:
            raise EssHipError(f'{fn}: {name} must be {" / ".join(str(d) for d in _EVCOL_DTYPES[name])} '
                              f'{list(t.shape)}, got {v.dtype}{tuple(v.shape)}')
    return t.shape[0], _int_in(fn, 'total', total, 0, t.shape[0])


def _formed_words(fn, named, dtype, shape):
    for name, v in named:
        if v.dtype != dtype or tuple(v.shape) != tuple(shape):
            raise EssHipError(f'{fn}: {name} must be {str(dtype).replace("torch.", "")} {list(shape)}, got {v.dtype}{tuple(v.shape)}')


def event_scatter_store(t, x, y, p, starts, counts, formats, acc, flavour, total, window_capacity, maps=None, map_of=None):
    """event_scatter_ring* on the device event store: the same sums, bit for bit, as the ring source leaves for the same events.
    t, x, y, p: device [capacity] flat columns (dtypes as event_ingest_columns; capacity a multiple of 16 up to 2^40), the first
    `total` events filled, recordings one behind the other.  starts: device int64 [n_slots], ABSOLUTE event indices; counts, formats:
    device int32 [n_slots] -- slot i's window is the counts[i] events from starts[i] on, nothing wraps.  A negative start,
    start + count > total, count > window_capacity, an unknown format bit (or map word): the slot counts as empty, its planes of
    acc stay as they are.  window_capacity (1 .. 2^22) shapes the launch, not the store's size.  acc: device int64 [n_slots, C, H, W],
    the sums are added to it.  flavour: EVENT_STORE_SIGNED / _SEPARATE / _HISTOGRAM (the EVENT_REP_* rules for C) or
    EVENT_STORE_TRILINEAR with maps, map_of as event_scatter_ring_trilinear takes them (refused with any other flavour).  -> acc"""
    return _event_call('event_scatter_store', 'store', 'store', (t, x, y, p), (starts, counts, formats), None, acc, 'none', flavour=flavour,
                       rectify=(maps, map_of), total=total, window_capacity=window_capacity)


def event_store_windows(t, table, recording, bounds, rule, sequence_steps, starts, counts, formats, flags, total, window_capacity,
                        n_per_window=None, sample_map=None, map_of=None):
    """A batch's sample table -> the B * T slot words event_scatter_store and event_grid_finish_window read, in one launch.
    t: the store's time column, device [capacity] int64 or float64; table: device int64 [n_recordings, 4] rows (begin, end, format,
    reserved), a negative format marks an unused row; recording: device int32 [B], the samples' rows; bounds: device int64 or
    float64 [B, 1] ([B, T + 1] under EVENT_STORE_RULE_DURATION), 8-byte words READ IN THE RECORDING'S OWN TIME TYPE (a recording of
    the other type than the tensor's dtype gets its words through .view()), prepared by the host as datasets.event_feed's rules
    prepare them; under EVENT_STORE_RULE_COUNT_INDEX bounds[b, 0] is the int64 end index relative to the recording.  rule,
    n_per_window, the three flag bits: as include/ess_hip.h states them.  starts (int64 [B T]), counts, formats (int32 [B T]) and flags
    (int32 [B]) are written for every sample; sample_map (int32 [B]) and map_of (int32 [B T]): both or neither.  -> flags"""
    fn = 'event_store_windows'
    T = _int_in(fn, 'sequence_steps', sequence_steps, 1, 65535)
    if isinstance(rule, bool) or rule not in _EVENT_STORE_RULES:
        raise EssHipError(f'{fn}: rule={rule!r} must be EVENT_STORE_RULE_COUNT_TIME, _COUNT_INDEX or _DURATION')
    if (sample_map is None) != (map_of is None):
        raise EssHipError(f'{fn}: sample_map and map_of are given together (the map words are passed through) or not at all')
    maps = () if map_of is None else (('sample_map', sample_map), ('map_of', map_of))
    named = (('t', t), ('table', table), ('recording', recording), ('bounds', bounds), ('starts', starts), ('counts', counts),
             ('formats', formats), ('flags', flags)) + maps
    _are_tensors(fn, named)
    if t.dim() != 1 or t.dtype not in _EVCOL_DTYPES['t'] or t.shape[0] < EVCOL_STRIDE_ALIGN or t.shape[0] % EVCOL_STRIDE_ALIGN or \
            t.shape[0] > EVENT_STORE_MAX_CAPACITY:
        raise EssHipError(f'{fn}: t must be int64 / float64 [capacity], capacity a multiple of {EVCOL_STRIDE_ALIGN} in '
                          f'[{EVCOL_STRIDE_ALIGN}, 2^40], got {t.dtype}{tuple(t.shape)}')
    total = _int_in(fn, 'total', total, 0, t.shape[0])
    window_capacity = _int_in(fn, 'window_capacity', window_capacity, 1, INGEST_MAX_CAPACITY)
    if rule == EVENT_STORE_RULE_DURATION:
        if n_per_window is not None:
            raise EssHipError(f'{fn}: n_per_window belongs to the count rules')
        n_per_window = 0
    else:
        n_per_window = _int_in(fn, 'n_per_window', n_per_window, 1, window_capacity)
    if table.dim() != 2 or table.dtype != torch.int64 or table.shape[0] < 1 or table.shape[1] != EVENT_STORE_TABLE_WORDS:
        raise EssHipError(f'{fn}: table must be int64 [n_recordings, {EVENT_STORE_TABLE_WORDS}] rows of (begin, end, format, reserved), '
                          f'got {table.dtype}{tuple(table.shape)}')
    if recording.dim() != 1 or recording.dtype != torch.int32 or not 1 <= recording.shape[0] * T <= 65535:
        raise EssHipError(f'{fn}: recording must be int32 [B] with B * sequence_steps in 1..65535, got {recording.dtype}{tuple(recording.shape)}')
    B = recording.shape[0]
    n_bounds = T + 1 if rule == EVENT_STORE_RULE_DURATION else 1
    if bounds.dtype not in (torch.int64, torch.float64) or tuple(bounds.shape) != (B, n_bounds):
        raise EssHipError(f'{fn}: bounds must be int64 / float64 [{B}, {n_bounds}], got {bounds.dtype}{tuple(bounds.shape)}')
    _formed_words(fn, (('starts', starts),), torch.int64, (B * T,))
    _formed_words(fn, (('counts', counts), ('formats', formats)) + maps[1:], torch.int32, (B * T,))
    _formed_words(fn, (('flags', flags),) + maps[:1], torch.int32, (B,))
    _on_device(fn, named)
    P = lambda v: c_void_p(0 if v is None else v.data_ptr())  # noqa: E731
    _check(lib().ess_event_store_windows(P(t), t.shape[0], total, P(table), table.shape[0], P(recording), P(bounds), P(sample_map), B, T,
                                         int(rule), n_per_window, window_capacity, P(starts), P(counts), P(formats), P(map_of), P(flags),
                                         stream()), 'ess_' + fn)
    return flags


def event_ingest_store(t, x, y, p, starts, counts, formats, out, flavour, total, window_capacity, masks=None, mask_of=None,
                       mask_size=None, maps=None, map_of=None, acc=None):
    """event_ingest_masked on the device event store: the four flavours, both halves, with or without hot-pixel masks.
    t .. formats, flavour, total, window_capacity, maps, map_of: as event_scatter_store takes them, with its slot refusals.
    out: fp32 [n_slots, C, H, W], returned -- the plain finish follows the scatter, the bits of event_ingest_ring* /
    event_ingest_ring_rep on the same events, acc (int64 [n_slots, C, H, W], all zero before; None: allocated and zeroed here) all zero again --
    or None: scatter only, acc (then required) keeps the sums for event_grid_finish*, and is returned.
    masks, mask_of, mask_size: as event_ingest_masked takes them -- a hot event is dropped on its raw (x, y) before a rectify map
    sees it, the window's time base comes from its first and last event whether masked or not, a mask word that is neither
    MASK_NONE nor in 0 .. n_masks - 1 leaves the slot empty.  masks=None and mask_of=None: event_scatter_store's sums, bit for bit."""
    return _event_call('event_ingest_store', 'store', 'store_masked', (t, x, y, p), (starts, counts, formats), out, acc, 'optional',
                       flavour=flavour, rectify=(maps, map_of), masks=(masks, mask_of, mask_size), total=total,
                       window_capacity=window_capacity)


def event_voxels(kind, cols, words, out, acc, representation=EVENT_REP_SIGNED, trilinear=False, maps=None, map_of=None, masks=None,
                 total=None, window_capacity=None):
    """The one route from a caller's configuration to the binding above that serves it; no kernel path and no check of its own.
    kind, cols, words: the source as _event_call takes it -- 'ring' (rows, starts, counts, formats), 'columns' (counts, formats) or
    'store' (starts, counts, formats), the latter with total and window_capacity.  out: the grids, or None: scatter only into acc.
    trilinear: the trilinear flavour with maps / map_of (handed on under trilinear alone), else `representation`.  masks: None, or
    (masks, mask_of, mask_size) of a caller that was configured with hot-pixel masks:
        masks                      -> event_ingest_masked, the store: event_ingest_store
        no masks, trilinear        -> event_ingest_<kind>_trilinear / event_scatter_ring_trilinear
        no masks, not signed       -> event_ingest_<kind>_rep / event_scatter_ring_rep
        no masks, signed           -> event_ingest_<kind> / event_scatter_ring
        the store without masks    -> event_scatter_store (out None), event_ingest_store"""
    if not trilinear:
        maps = map_of = None
    if kind == 'store':
        flavour = EVENT_STORE_TRILINEAR if trilinear else representation
        if masks is None and out is None:
            return event_scatter_store(*cols, *words, acc, flavour, total, window_capacity, maps, map_of)
        m = (None, None, None) if masks is None else masks
        return event_ingest_store(*cols, *words, out, flavour, total, window_capacity, masks=m[0], mask_of=m[1], mask_size=m[2], maps=maps,
                                  map_of=map_of, acc=acc)
    if masks is not None:
        rows, starts = words[:2] if kind == 'ring' else (None, None)
        return event_ingest_masked(*cols, rows, starts, *words[-2:], out, *masks, representation=representation, trilinear=trilinear,
                                   maps=maps, map_of=map_of, acc=acc)
    if out is None and kind != 'ring':
        raise EssHipError(f"event_voxels: out=None (scatter only) without masks is the ring's and the store's (kind={kind!r})")
    name = f'event_ingest_{kind}' if out is not None else 'event_scatter_ring'
    grids = (acc,) if out is None else (out,)
    after = () if out is None else (acc,)
    if trilinear:
        return globals()[name + '_trilinear'](*cols, *words, *grids, maps, map_of, *after)
    if representation != EVENT_REP_SIGNED:
        return globals()[name + '_rep'](*cols, *words, *grids, representation, *after)
    return globals()[name](*cols, *words, *grids, *after)


def event_store_pixel_counts(x, y, begins, ends, formats, counts, total):
    """Plain per-pixel event counts of index ranges of the device event store.  x, y: the store's coordinate columns, device int16 /
    uint16 [capacity].  begins, ends: device int64 [n], ABSOLUTE event indices, job j counts the events begins[j] .. ends[j] - 1;
    formats: device int32 [n], the EVCOL_* word the job's coordinates are decoded under.  counts: device int64 [n, H, W], ADDED TO
    and returned: one per event whose decoded (x, y) lies inside H x W, both polarities together, whatever the range's length (no
    2^22 bound: these are not the ingest's scaled sums).  A range outside [0, total], begin > end or an unknown format bit: the job
    counts nothing.  One launch shaped by the capacity and n alone, every word read on the device: capturable."""
    fn = 'event_store_pixel_counts'
    named = (('x', x), ('y', y), ('begins', begins), ('ends', ends), ('formats', formats), ('counts', counts))
    _are_tensors(fn, named)
    if x.dim() != 1 or x.shape[0] < EVCOL_STRIDE_ALIGN or x.shape[0] % EVCOL_STRIDE_ALIGN or x.shape[0] > EVENT_STORE_MAX_CAPACITY:
        raise EssHipError(f'{fn}: x must be [capacity], capacity a multiple of {EVCOL_STRIDE_ALIGN} in [{EVCOL_STRIDE_ALIGN}, 2^40], '
                          f'got {tuple(x.shape)}')
    for name, v in named[:2]:
        if v.dtype not in _EVCOL_DTYPES[name] or v.shape != x.shape:
            raise EssHipError(f'{fn}: {name} must be {" / ".join(str(d) for d in _EVCOL_DTYPES[name])} '
                              f'{list(x.shape)}, got {v.dtype}{tuple(v.shape)}')
    total = _int_in(fn, 'total', total, 0, x.shape[0])
    if counts.dim() != 3 or counts.dtype != torch.int64 or counts.numel() == 0 or not 1 <= counts.shape[0] <= 65535 or \
            counts.shape[1] > MASK_MAX_SIDE or counts.shape[2] > MASK_MAX_SIDE:
        raise EssHipError(f'{fn}: counts must be a non-empty int64 [n, H, W] tensor, n in 1..65535, H and W in 1..{MASK_MAX_SIDE}, '
                          f'got {counts.dtype}{tuple(counts.shape)}')
    n, H, W = counts.shape
    _formed_words(fn, named[2:4], torch.int64, (n,))
    _formed_words(fn, named[4:5], torch.int32, (n,))
    _on_device(fn, named)
    _check(lib().ess_event_store_pixel_counts(c_void_p(x.data_ptr()), c_void_p(y.data_ptr()), x.shape[0], total, ptr(begins, torch.int64),
                                              ptr(ends, torch.int64), ptr(formats, torch.int32), n, H, W, c_void_p(counts.data_ptr()),
                                              stream()), 'ess_' + fn)
    return counts


def event_count_mask(counts, thresholds, masks, mode=MASK_REPLACE):
    """event_hot_pixel_mask's rule on PLAIN counts.  counts: device int64 [n, H, W], what event_store_pixel_counts leaves (one per
    event, no 2^40 scale, read only).  thresholds: device int64 [n], in events: >= 0 -- bit (y, x) of masks[i] is set iff
    counts[i, y, x] > thresholds[i]; < 0 -- masks[i] is neither read nor written.  masks, mode: as event_hot_pixel_mask takes them
    (the same kernel, the same word layout and tail-bit rule).  -> masks"""
    fn = 'event_count_mask'
    named = (('counts', counts), ('thresholds', thresholds), ('masks', masks))
    _are_tensors(fn, named)
    if counts.dim() != 3 or counts.dtype != torch.int64 or counts.numel() == 0:
        raise EssHipError(f'{fn}: counts must be a non-empty int64 [n, H, W] tensor (plain per-pixel counts), '
                          f'got {counts.dtype}{tuple(counts.shape)}')
    n, H, W = counts.shape
    if H > MASK_MAX_SIDE or W > MASK_MAX_SIDE:
        raise EssHipError(f'{fn}: counts of {H} x {W} pixels: a side is 1..{MASK_MAX_SIDE}')
    if thresholds.dtype != torch.int64 or tuple(thresholds.shape) != (n,):
        raise EssHipError(f'{fn}: thresholds must be int64 [{n}], got {thresholds.dtype}{tuple(thresholds.shape)}')
    if _mask_tensor(fn, masks, (H, W), n)[0] != n:
        raise EssHipError(f'{fn}: masks must hold {n} masks, one per plane of counts, got {tuple(masks.shape)}')
    if isinstance(mode, bool) or mode not in (MASK_REPLACE, MASK_OR):
        raise EssHipError(f'{fn}: mode={mode!r} must be MASK_REPLACE or MASK_OR')
    _on_device(fn, named)
    _check(lib().ess_event_count_mask(c_void_p(counts.data_ptr()), n, H, W, c_void_p(thresholds.data_ptr()), c_void_p(masks.data_ptr()),
                                      int(mode), stream()), 'ess_' + fn)
    return masks


def event_grid_finish(counts, acc, out, crop_rows=None, resize=None, normalize=GRID_NORM_NONE):
    """The second half: acc (device int64 [n_slots, bins, Hs, Ws], the sums event_scatter_ring* left) -> out (fp32
    [n_slots, bins, out_rows, Wr], returned), the grid a reference LOADER hands the network.  Per slot, in this order: the sums are
    dequantised; normalize (GRID_NORM_NONE / GRID_NORM_UNBIASED: VoxelGrid(normalize=True) / GRID_NORM_POPULATION:
    normalize_voxel_grid) over the non-zero voxels of ALL Hs rows, with exact integer count and sum and an fp64 sum of squares in a
    fixed order; rows [0, crop_rows) are kept (None: Hs); they are resized bilinearly (align_corners=True, torch's fp32 coordinates)
    to resize=(Hr, Wr) (None: (crop_rows, Ws)); rows [0, out_rows) of that are stored -- out's shape names out_rows <= Hr and Wr.
    counts: device int32 [n_slots] -- INGEST_KEEP (< 0): out[i] is neither read nor written.  acc is ALL ZERO behind the call.  out is
    a pure function of the sums: the same bits run to run, for a slot alone or among others; with no crop, no resize and no
    normalisation they are event_ingest_ring's bits.  No memset, no synchronisation: capturable."""
    fn = 'event_grid_finish'
    named = (('counts', counts), ('acc', acc), ('out', out))
    _are_tensors(fn, named)
    n_slots, bins, Hs, Ws, crop_rows, Hr, Wr = _finish_geometry(fn, counts, acc, out, crop_rows, resize, normalize, window=False)
    _on_device(fn, named)
    ws = grid_finish_workspace(n_slots, bins, Hs, Ws, out.device)
    _check(lib().ess_event_grid_finish(ptr(counts, torch.int32), n_slots, bins, Hs, Ws, c_void_p(acc.data_ptr()), acc.numel() * 8,
                                       crop_rows, Hr, Wr, out.shape[2], int(normalize), c_void_p(out.data_ptr()),
                                       c_void_p(ws.data_ptr()), ws.numel(), stream()), 'ess_event_grid_finish')
    return out


def _resize_pair(fn, resize):
    if not isinstance(resize, (tuple, list)) or len(resize) != 2 or \
            any(isinstance(v, bool) or not isinstance(v, int) or v < 1 or v > 1 << 24 for v in resize):
        raise EssHipError(f'{fn}: resize={resize!r} must be a pair of positive ints (Hr, Wr)')
    return resize


def _finish_geometry(fn, counts, acc, out, crop_rows, resize, normalize, window):
    """What the two loader finishes check of acc, crop_rows, resize, out, normalize and counts, in this order -> (n_slots, bins, Hs,
    Ws, crop_rows, Hr, Wr) with the defaults filled in.  window: out is a window inside the Hr x Wr grid, else its rows <= Hr."""
    n_slots, bins, Hs, Ws = _finish_acc(fn, acc, 'Hs, Ws')
    crop_rows = Hs if crop_rows is None else crop_rows
    if isinstance(crop_rows, bool) or not isinstance(crop_rows, int) or not 1 <= crop_rows <= Hs:
        raise EssHipError(f'{fn}: crop_rows={crop_rows!r} must be an int in [1, {Hs}]')
    Hr, Wr = _resize_pair(fn, (crop_rows, Ws) if resize is None else resize)
    if out.dim() != 4 or out.dtype != torch.float32 or out.numel() == 0 or out.shape[0] != n_slots or out.shape[1] != bins \
            or out.shape[2] > Hr or (out.shape[3] > Wr if window else out.shape[3] != Wr):
        form = f'h <= {Hr}, w <= {Wr}] (the window inside the {Hr} x {Wr} grid)' if window else f'rows <= {Hr}, {Wr}]'
        raise EssHipError(f'{fn}: out must be fp32 [{n_slots}, {bins}, {form}, got {out.dtype}{tuple(out.shape)}')
    if normalize not in (GRID_NORM_NONE, GRID_NORM_UNBIASED, GRID_NORM_POPULATION) or isinstance(normalize, bool):
        raise EssHipError(f'{fn}: normalize={normalize!r} must be GRID_NORM_NONE, GRID_NORM_UNBIASED or GRID_NORM_POPULATION')
    if counts.dtype != torch.int32 or tuple(counts.shape) != (n_slots,):
        raise EssHipError(f'{fn}: counts must be int32 [{n_slots}], got {counts.dtype}{tuple(counts.shape)}')
    return n_slots, bins, Hs, Ws, crop_rows, Hr, Wr


def grid_finish_workspace(n_slots, bins, Hs, Ws, device):
    """The cached buffer event_grid_finish takes its statistics from.  Every call writes what it reads of it; the tests fill it with
    0xFF bytes before a launch to prove that."""
    return workspace(lib().ess_event_grid_finish_workspace(n_slots, bins, Hs, Ws), device, 'grid_finish')


def _window_words(fn, words, n_groups):
    """the (flip, y0, x0, reserved) table of the training window: int32 [n_groups, 4]"""
    if words.dtype != torch.int32 or tuple(words.shape) != (n_groups, 4):
        raise EssHipError(f'{fn}: words must be int32 [{n_groups}, 4] rows of (flip, y0, x0, reserved), got {words.dtype}{tuple(words.shape)}')


def event_grid_finish_window(counts, acc, out, words, slots_per_group, crop_rows=None, resize=None, normalize=GRID_NORM_NONE):
    """event_grid_finish with the loaders' training augmentation fused into its map pass: counts, acc, crop_rows, resize, normalize as
    there; call the grid it would store g [n_slots, bins, rows, Wr] -- rows = Hr here: out's shape names the WINDOW.  out: fp32
    [n_slots, bins, h <= Hr, w <= Wr] (returned); words: device int32 [ceil(n_slots / slots_per_group), 4] rows of (flip, y0, x0,
    reserved), slot i reads row i // slots_per_group (the T windows of a sample share one row, and so does label_window):
        out[i, b, y, x] = g[i, b, y0 + y, Wr - 1 - (x0 + x) if flip else x0 + x]
    the flip first, then the crop (albumentations' order); only the window's voxels are computed.  The device reads flip as != 0 and
    clamps y0 into [0, Hr - h] and x0 into [0, Wr - w].  The bits are event_grid_finish's followed by torch.flip and slicing; acc is
    ALL ZERO behind the call, the sums no output read included.  No memset, no synchronisation: capturable."""
    fn = 'event_grid_finish_window'
    named = (('counts', counts), ('acc', acc), ('out', out), ('words', words))
    _are_tensors(fn, named)
    n_slots, bins, Hs, Ws, crop_rows, Hr, Wr = _finish_geometry(fn, counts, acc, out, crop_rows, resize, normalize, window=True)
    if isinstance(slots_per_group, bool) or not isinstance(slots_per_group, int) or slots_per_group < 1:
        raise EssHipError(f'{fn}: slots_per_group={slots_per_group!r} must be a positive int')
    _window_words(fn, words, -(-n_slots // slots_per_group))
    _on_device(fn, named)
    ws = grid_finish_workspace(n_slots, bins, Hs, Ws, out.device)
    _check(lib().ess_event_grid_finish_window(ptr(counts, torch.int32), n_slots, bins, Hs, Ws, c_void_p(acc.data_ptr()), acc.numel() * 8,
                                              crop_rows, Hr, Wr, Hr, int(normalize), ptr(words, torch.int32), slots_per_group,
                                              out.shape[2], out.shape[3], c_void_p(out.data_ptr()), c_void_p(ws.data_ptr()), ws.numel(),
                                              stream()), 'ess_event_grid_finish_window')
    return out


def label_window(src, out, words, resize=None):
    """The label's side of event_grid_finish_window.  src: device uint8 [n, Hs, Ws]; resize=(Hr, Wr) (None: (Hs, Ws)): nearest resize
    by the exact integer rule sy = min(dy * Hs // Hr, Hs - 1), sx alike; then the flip and the window of sample i's row words[i]
    (device int32 [n, 4] = (flip, y0, x0, reserved), clamped on the device as there) -> out int64 [n, h <= Hr, w <= Wr] (returned).
    Values pass unchanged: 255 stays 255.  The loaders resize labels with cv2.resize(INTER_NEAREST), which computes
    floor(d * (1 / (dst / src))) in doubles; the two rules agree for every d at 440 -> 448, 640 -> 640, 346 -> 352 and 480 -> 448,
    but parity with cv2 itself is UNPINNED (cv2 is not a dependency), as datasets/augment.py says of albumentations."""
    fn = 'label_window'
    named = (('src', src), ('out', out), ('words', words))
    _are_tensors(fn, named)
    if src.dim() != 3 or src.dtype != torch.uint8 or src.numel() == 0 or src.shape[0] > 65535:
        raise EssHipError(f'{fn}: src must be a non-empty uint8 [n <= 65535, Hs, Ws] tensor, got {src.dtype}{tuple(src.shape)}')
    n, Hs, Ws = src.shape
    Hr, Wr = _resize_pair(fn, (Hs, Ws) if resize is None else resize)
    if out.dim() != 3 or out.dtype != torch.int64 or out.numel() == 0 or out.shape[0] != n or out.shape[1] > Hr or out.shape[2] > Wr:
        raise EssHipError(f'{fn}: out must be int64 [{n}, h <= {Hr}, w <= {Wr}] (the window inside the {Hr} x {Wr} label), '
                          f'got {out.dtype}{tuple(out.shape)}')
    _window_words(fn, words, n)
    _on_device(fn, named)
    _check(lib().ess_label_window(ptr(src, torch.uint8), n, Hs, Ws, Hr, Wr, ptr(words, torch.int32), out.shape[1], out.shape[2],
                                  ptr(out, torch.int64), stream()), 'ess_label_window')
    return out


def voxel_normalize_(grids, mode):
    """In-place per-slice (dim 0) normalisation over the non-zero voxels; mode 0 = VoxelGrid, 1 = normalize_voxel_grid."""
    ns = grids.shape[0]
    L = lib()
    nbytes = L.ess_voxel_normalize_workspace(ns)
    ws = workspace(nbytes, grids.device, 'voxnorm')
    _check(L.ess_voxel_normalize(ptr(grids), ns, grids[0].numel(), mode, c_void_p(ws.data_ptr()), nbytes, stream()),
           'ess_voxel_normalize')
    return grids


# ------------------------------------------------------------------------------------------ losses / optimiser / metrics
def task_loss(logits, labels, want_grad, scale=1.0, ignore_index=255, use_dice=True, use_ce=True):
    N, K, H, W = logits.shape
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    dz = torch.empty_like(logits) if want_grad else None
    ws = workspace(lib().ess_task_loss_workspace(K), logits.device, 'loss')
    _check(lib().ess_task_loss(ptr(logits), ptr(labels, torch.int64), ptr(loss), ptr(dz), c_float(scale), N, K, H * W,
                               int(ignore_index), int(use_dice), int(use_ce), c_void_p(ws.data_ptr()), c_size_t(ws.numel()), stream()),
           'ess_task_loss')
    return loss, dz


def sym_js_loss(a, b, want_grad, scale=1.0):
    N, K, H, W = a.shape
    loss = torch.empty((), dtype=torch.float32, device=a.device)
    da = torch.empty_like(a) if want_grad else None
    ws = _mean_loss_ws(a.device)
    _check(lib().ess_sym_js_loss(ptr(a), ptr(b), ptr(loss), ptr(da), c_float(scale), N, K, H * W, c_void_p(ws.data_ptr()),
                                 c_size_t(ws.numel()), stream()), 'ess_sym_js_loss')
    return loss, da


def l1_loss(a, b, want_grad, scale=1.0):
    loss = torch.empty((), dtype=torch.float32, device=a.device)
    da = torch.empty_like(a) if want_grad else None
    ws = _mean_loss_ws(a.device)
    _check(lib().ess_l1_loss(ptr(a), ptr(b), ptr(loss), ptr(da), c_float(scale), a.numel(), c_void_p(ws.data_ptr()),
                             c_size_t(ws.numel()), stream()), 'ess_l1_loss')
    return loss, da


def l1_loss_c8(a, b, n_real, want_grad, scale=1.0):
    """L1 mean over two BF16_C8 tensors; n_real = N*C*H*W real elements (the mean's denominator)."""
    if a.shape != b.shape:
        raise EssHipError('l1_loss_c8: shape mismatch')
    loss = torch.empty((), dtype=torch.float32, device=a.device)
    da = torch.empty_like(a) if want_grad else None
    ws = _mean_loss_ws(a.device)
    _check(lib().ess_l1_loss_c8(ptr(a, torch.bfloat16), ptr(b, torch.bfloat16), ptr(loss), ptr(da, torch.bfloat16), c_float(scale),
                                a.numel() // 8, int(n_real), c_void_p(ws.data_ptr()), c_size_t(ws.numel()), stream()), 'ess_l1_loss_c8')
    return loss, da


def augment_image_label(img, label, params, height, width, id_lut=None):
    """Batch augmentation in one launch (ess_augment_image_label).  img fp32 [N, Hs, Ws] on the 0..255 scale, label int64
    [N, Hs, Ws] or None, params fp32 [N, 12] (datasets/augment.py draws them) -> (fp32 [N, 1, H, W] in [0, 1], int64 [N, H, W])."""
    N, Hs, Ws = img.shape
    if params.shape != (N, 12):
        raise EssHipError('augment_image_label: params must be [N, 12]')
    if id_lut is not None and id_lut.numel() < 256:
        raise EssHipError('augment_image_label: id_lut must have 256 entries (the kernel indexes it with the label id clamped to 0..255)')
    out = torch.empty(N, 1, height, width, dtype=torch.float32, device=img.device)
    out_l = torch.empty(N, height, width, dtype=torch.int64, device=img.device) if label is not None else None
    _check(lib().ess_augment_image_label(ptr(img), ptr(label, torch.int64), ptr(params), ptr(id_lut, torch.int64), ptr(out),
                                         ptr(out_l, torch.int64), N, Hs, Ws, height, width, stream()), 'ess_augment_image_label')
    return out, out_l


IMAGE_MAX_TAPS = 33     # ESS_IMAGE_MAX_TAPS: 2 * ceil(in / out) + 1 coefficients a window at the most, a side shrinks by at most 16
IMAGE_MAX_SIDE = 32768  # ESS_IMAGE_MAX_SIDE


def _image_table(fn, name, t, n_in, n_out):
    """a pass's table [2 + taps, n_out] (datasets.image_store.pil_bilinear_tables), None exactly where the size stays -> taps"""
    if n_in == n_out:
        if t is not None:
            raise EssHipError(f'{fn}: {name} belongs to a pass that changes the size; {n_in} -> {n_out} is skipped, as PIL skips it: pass None')
        return 0
    if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != n_out or not 3 <= t.shape[0] <= 2 + IMAGE_MAX_TAPS \
            or not t.is_contiguous():
        got = f'{t.dtype}{tuple(t.shape)}' if torch.is_tensor(t) else type(t).__name__
        raise EssHipError(f'{fn}: {name} must be a contiguous int32 [2 + taps, {n_out}] table with taps <= {IMAGE_MAX_TAPS} for the pass '
                          f'{n_in} -> {n_out}, got {got}')
    return t.shape[0] - 2


def image_ingest(frame, out, h_table=None, v_table=None, scratch=None, standardize=False, minmax=None, label=None, label_rows=None,
                 label_cols=None, out_label=None):
    """One decoded frame -> its store slot (ess_image_ingest), in PIL's integer arithmetic: frame uint8 [H, W, 3] (RGB; convert('L'))
    or [H, W] (gray) -> out uint8 [Hr, Wr] = Image.resize((Wr, Hr), BILINEAR) of the gray frame.  h_table / v_table: the passes'
    int32 [2 + taps, Wr] / [2 + taps, Hr] tables of datasets.image_store.pil_bilinear_tables, None exactly where the size stays.
    scratch: uint8 [H, Wr] (RGB input or a horizontal pass; allocated when None).  minmax: int32 [2], receives the resized frame's
    min and max; standardize=True (needs it) then stretches v -> trunc(255.0 (v - min) / (max - min)), a constant frame to 0.
    label uint8 [H, W] with label_rows int32 [Hr], label_cols int32 [Wr] (pil_nearest_table) -> out_label uint8 [Hr, Wr].
    Returns out.  Everything is checked before a pointer is taken."""
    fn = 'image_ingest'
    if not torch.is_tensor(frame) or frame.dtype != torch.uint8 or frame.dim() not in (2, 3) or (frame.dim() == 3 and frame.shape[2] != 3) \
            or frame.numel() == 0 or not frame.is_contiguous():
        got = f'{frame.dtype}{tuple(frame.shape)}' if torch.is_tensor(frame) else type(frame).__name__
        raise EssHipError(f'{fn}: frame must be a non-empty contiguous uint8 [H, W, 3] (RGB) or [H, W] (gray) tensor, got {got}')
    H, W = int(frame.shape[0]), int(frame.shape[1])
    channels = 3 if frame.dim() == 3 else 1
    if not torch.is_tensor(out) or out.dtype != torch.uint8 or out.dim() != 2 or out.numel() == 0 or not out.is_contiguous():
        got = f'{out.dtype}{tuple(out.shape)}' if torch.is_tensor(out) else type(out).__name__
        raise EssHipError(f'{fn}: out must be a non-empty contiguous uint8 [Hr, Wr] tensor, got {got}')
    Hr, Wr = int(out.shape[0]), int(out.shape[1])
    if max(H, W, Hr, Wr) > IMAGE_MAX_SIDE:
        raise EssHipError(f'{fn}: source {H} x {W}, slot {Hr} x {Wr}: a side is at most {IMAGE_MAX_SIDE}')
    h_taps, v_taps = _image_table(fn, 'h_table', h_table, W, Wr), _image_table(fn, 'v_table', v_table, H, Hr)
    tensors = [('frame', frame), ('out', out)] + [(n, t) for n, t in (('h_table', h_table), ('v_table', v_table)) if t is not None]
    need_scratch = channels == 3 or h_table is not None
    if scratch is not None:
        tensors.append(('scratch', _formed(fn, 'scratch', scratch, torch.uint8, (H, Wr))))
    if minmax is not None:
        tensors.append(('minmax', _formed(fn, 'minmax', minmax, torch.int32, (2,))))
    elif standardize:
        raise EssHipError(f'{fn}: standardize needs minmax, an int32 [2] tensor for the frame\'s min and max')
    if (label is None) != (out_label is None) or (label is None) != (label_rows is None) or (label is None) != (label_cols is None):
        raise EssHipError(f'{fn}: label, label_rows, label_cols and out_label are given together or not at all')
    if label is not None:
        tensors += [('label', _formed(fn, 'label', label, torch.uint8, (H, W))), ('label_rows', _formed(fn, 'label_rows', label_rows, torch.int32, (Hr,))),
                    ('label_cols', _formed(fn, 'label_cols', label_cols, torch.int32, (Wr,))),
                    ('out_label', _formed(fn, 'out_label', out_label, torch.uint8, (Hr, Wr)))]
    _on_device(fn, tensors)
    if any(t.device != frame.device for _, t in tensors):
        raise EssHipError(f'{fn}: every tensor must lie on the frame\'s device ({frame.device})')
    if scratch is None and need_scratch:
        scratch = torch.empty(H, Wr, dtype=torch.uint8, device=frame.device)
    _check(lib().ess_image_ingest(ptr(frame, torch.uint8), channels, H, W, ptr(h_table, torch.int32), h_taps, ptr(v_table, torch.int32), v_taps,
                                  ptr(scratch if need_scratch else None, torch.uint8), ptr(out, torch.uint8), Hr, Wr, int(bool(standardize)),
                                  ptr(minmax, torch.int32), ptr(label, torch.uint8), ptr(label_rows, torch.int32), ptr(label_cols, torch.int32),
                                  ptr(out_label, torch.uint8), stream()), 'ess_image_ingest')
    return out


def image_ingest_frame(frame, out, h_table=None, v_table=None, scratch=None, resized_rows=None, gray_last=True):
    """One paired camera frame of an event loader -> its store slot (ess_image_ingest_frame), in PIL's integer arithmetic: frame uint8
    [H, W, 3] or [H, W] -> out uint8 [out_rows, Wr], the top out_rows rows of Image.resize((Wr, Hr)) -- with the tables of
    datasets.image_store.pil_resize_tables, bicubic as the loaders' default filter is -- and, for an RGB frame, convert('L') BEHIND the
    resize (gray_last=True, the loaders' order) or in front of it (False: image_ingest's bits).  resized_rows: Hr (default: out_rows,
    nothing cut).  h_table / v_table: int32 [2 + taps, Wr] / [2 + taps, Hr], None exactly where the side stays.  scratch: uint8
    [H, Wr, 3] (RGB, gray last) or [H, Wr], needed with a horizontal pass (or gray first); allocated when None.  Returns out.
    Everything is checked before a pointer is taken."""
    fn = 'image_ingest_frame'
    if not torch.is_tensor(frame) or frame.dtype != torch.uint8 or frame.dim() not in (2, 3) or (frame.dim() == 3 and frame.shape[2] != 3) \
            or frame.numel() == 0 or not frame.is_contiguous():
        got = f'{frame.dtype}{tuple(frame.shape)}' if torch.is_tensor(frame) else type(frame).__name__
        raise EssHipError(f'{fn}: frame must be a non-empty contiguous uint8 [H, W, 3] (RGB) or [H, W] (gray) tensor, got {got}')
    H, W = int(frame.shape[0]), int(frame.shape[1])
    channels = 3 if frame.dim() == 3 else 1
    if not torch.is_tensor(out) or out.dtype != torch.uint8 or out.dim() != 2 or out.numel() == 0 or not out.is_contiguous():
        got = f'{out.dtype}{tuple(out.shape)}' if torch.is_tensor(out) else type(out).__name__
        raise EssHipError(f'{fn}: out must be a non-empty contiguous uint8 [out_rows, Wr] tensor, got {got}')
    out_rows, Wr = int(out.shape[0]), int(out.shape[1])
    Hr = out_rows if resized_rows is None else resized_rows
    if isinstance(Hr, bool) or not isinstance(Hr, (int, np.integer)) or Hr < out_rows:
        raise EssHipError(f'{fn}: resized_rows={Hr!r}: the rows of the resized frame, an int >= out\'s {out_rows} rows')
    Hr = int(Hr)
    if max(H, W, Hr, Wr) > IMAGE_MAX_SIDE:
        raise EssHipError(f'{fn}: source {H} x {W}, resized {Hr} x {Wr}: a side is at most {IMAGE_MAX_SIDE}')
    if not isinstance(gray_last, (bool, int, np.integer)) or gray_last not in (0, 1):
        raise EssHipError(f'{fn}: gray_last={gray_last!r} must be True or False')
    h_taps, v_taps = _image_table(fn, 'h_table', h_table, W, Wr), _image_table(fn, 'v_table', v_table, H, Hr)
    tensors = [('frame', frame), ('out', out)] + [(n, t) for n, t in (('h_table', h_table), ('v_table', v_table)) if t is not None]
    rgb_last = channels == 3 and bool(gray_last)
    need_scratch = h_table is not None or (channels == 3 and not rgb_last)
    scratch_shape = (H, Wr, 3) if rgb_last else (H, Wr)
    if scratch is not None:
        tensors.append(('scratch', _formed(fn, 'scratch', scratch, torch.uint8, scratch_shape)))
    _on_device(fn, tensors)
    if any(t.device != frame.device for _, t in tensors):
        raise EssHipError(f'{fn}: every tensor must lie on the frame\'s device ({frame.device})')
    if scratch is None and need_scratch:
        scratch = torch.empty(scratch_shape, dtype=torch.uint8, device=frame.device)
    _check(lib().ess_image_ingest_frame(ptr(frame, torch.uint8), channels, H, W, ptr(h_table, torch.int32), h_taps, ptr(v_table, torch.int32),
                                        v_taps, ptr(scratch if need_scratch else None, torch.uint8), ptr(out, torch.uint8), Hr, Wr, out_rows,
                                        int(bool(gray_last)), stream()), 'ess_image_ingest_frame')
    return out


def image_gather_unit(images, index, out=None):
    """transforms.ToTensor() on stored frames (ess_image_gather_unit): images uint8 [capacity, Hs, Ws], index int32 or int64 [B] on the
    device (read there: the launch is capturable) -> out fp32 [B, 1, Hs, Ws] = images[index] / 255, the bits of
    torch.from_numpy(u8).float().div(255) on the host; an index outside [0, capacity) gives an all-zero frame."""
    fn = 'image_gather_unit'
    if not torch.is_tensor(images) or images.dtype != torch.uint8 or images.dim() != 3 or images.numel() == 0 or not images.is_contiguous():
        got = f'{images.dtype}{tuple(images.shape)}' if torch.is_tensor(images) else type(images).__name__
        raise EssHipError(f'{fn}: images must be a non-empty contiguous uint8 [capacity, Hs, Ws] tensor, got {got}')
    capacity, Hs, Ws = (int(v) for v in images.shape)
    if max(Hs, Ws) > IMAGE_MAX_SIDE:
        raise EssHipError(f'{fn}: slots of {Hs} x {Ws}: a side is at most {IMAGE_MAX_SIDE}')
    if not torch.is_tensor(index) or index.dtype not in (torch.int32, torch.int64) or index.dim() != 1 or not 1 <= index.numel() <= 65535 \
            or not index.is_contiguous():
        got = f'{index.dtype}{tuple(index.shape)}' if torch.is_tensor(index) else type(index).__name__
        raise EssHipError(f'{fn}: index must be a contiguous int32 or int64 [B] tensor with 1 <= B <= 65535, got {got}')
    B = int(index.shape[0])
    tensors = [('images', images), ('index', index)]
    if out is not None:
        tensors.append(('out', _formed(fn, 'out', out, torch.float32, (B, 1, Hs, Ws))))
    _on_device(fn, tensors)
    if any(t.device != images.device for _, t in tensors):
        raise EssHipError(f'{fn}: every tensor must lie on the store\'s device ({images.device})')
    if out is None:
        out = torch.empty(B, 1, Hs, Ws, dtype=torch.float32, device=images.device)
    _check(lib().ess_image_gather_unit(ptr(images, torch.uint8), capacity, Hs, Ws, ptr(index, index.dtype), int(index.dtype == torch.int64), B,
                                       ptr(out), stream()), 'ess_image_gather_unit')
    return out


def augment_image_label_store(images, labels, index, rows, params, height, width, id_lut=None, out=None):
    """Stage 1 of the augmentation (ess_augment_image_label_store: augment_image_label's kernel body with another pixel source) reading
    the uint8 slots of an ImageStore through an index: images uint8 [n_slots, Hr, Wr], labels uint8 of the same shape or None,
    index int32 [B] on the device (a word outside the slots: an all-zero sample), rows: the top rows of a slot that exist (the loader's
    img[:height]), params fp32 [B, 12] -> (fp32 [B, 1, height, width] in [0, 1], int64 [B, height, width] or None): the bits of
    augment_image_label(images[index][:, :rows].float(), labels[index][:, :rows].long(), params, height, width, id_lut), with no float
    copy of the source.  out=(img, label): the tensors to fill."""
    fn = 'augment_image_label_store'
    if not torch.is_tensor(images) or images.dtype != torch.uint8 or images.dim() != 3 or images.numel() == 0 or not images.is_contiguous():
        got = f'{images.dtype}{tuple(images.shape)}' if torch.is_tensor(images) else type(images).__name__
        raise EssHipError(f'{fn}: images must be a non-empty contiguous uint8 [n_slots, Hr, Wr] tensor, got {got}')
    n_slots, Hr, Wr = (int(v) for v in images.shape)
    if labels is not None:
        _formed(fn, 'labels', labels, torch.uint8, (n_slots, Hr, Wr))
    if not torch.is_tensor(index) or index.dtype != torch.int32 or index.dim() != 1 or index.numel() == 0 or not index.is_contiguous():
        got = f'{index.dtype}{tuple(index.shape)}' if torch.is_tensor(index) else type(index).__name__
        raise EssHipError(f'{fn}: index must be a non-empty contiguous int32 [B] tensor, got {got}')
    B = int(index.shape[0])
    if isinstance(rows, bool) or not isinstance(rows, (int, np.integer)) or not 1 <= rows <= Hr:
        raise EssHipError(f'{fn}: rows={rows!r} must be an int in [1, {Hr}]: the top rows of a slot')
    for name, v in (('height', height), ('width', width)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= IMAGE_MAX_SIDE:
            raise EssHipError(f'{fn}: {name}={v!r} must be an int in [1, {IMAGE_MAX_SIDE}]')
    _formed(fn, 'params', params, torch.float32, (B, 12))
    if id_lut is not None and (not torch.is_tensor(id_lut) or id_lut.dtype != torch.int64 or id_lut.numel() < 256 or not id_lut.is_contiguous()):
        raise EssHipError(f'{fn}: id_lut must be a contiguous int64 tensor of 256 entries (the kernel indexes it with the label id)')
    tensors = [('images', images), ('index', index), ('params', params)] + [(n, t) for n, t in (('labels', labels), ('id_lut', id_lut)) if t is not None]
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2 or (out[1] is None) != (labels is None):
            raise EssHipError(f'{fn}: out must be (img, label) with a label tensor exactly where labels are given')
        tensors.append(('out[0]', _formed(fn, 'out[0]', out[0], torch.float32, (B, 1, height, width))))
        if labels is not None:
            tensors.append(('out[1]', _formed(fn, 'out[1]', out[1], torch.int64, (B, height, width))))
    _on_device(fn, tensors)
    if any(t.device != images.device for _, t in tensors):
        raise EssHipError(f'{fn}: every tensor must lie on the store\'s device ({images.device})')
    if out is None:
        out = (torch.empty(B, 1, height, width, dtype=torch.float32, device=images.device),
               torch.empty(B, height, width, dtype=torch.int64, device=images.device) if labels is not None else None)
    _check(lib().ess_augment_image_label_store(ptr(images, torch.uint8), ptr(labels, torch.uint8), ptr(index, torch.int32), n_slots, Hr, Wr,
                                               int(rows), ptr(params), ptr(id_lut, torch.int64), ptr(out[0]), ptr(out[1], torch.int64), B,
                                               int(height), int(width), stream()), 'ess_augment_image_label_store')
    return out[0], out[1]


def augment_perspective_filter(img, label, params, id_lut=None, out=None, scratch=None):
    """Second augmentation stage (ess_augment_perspective_filter): Perspective, brightness / contrast, the Sharpen / Blur /
    MotionBlur stencil.  img fp32 [N, 1, H, W] in [0, 1] (stage 1's output), label int64 [N, H, W] raw ids or None, params fp32
    [N, 24] (datasets/augment.py draws them) -> (fp32 [N, 1, H, W], int64 [N, H, W]).  out=(img, label) and scratch= (fp32 [N, H, W]):
    the tensors to fill and the stage's workspace, for a caller with static buffers (allocated here when None)."""
    N, _, H, W = img.shape
    if params.shape != (N, 24):
        raise EssHipError('augment_perspective_filter: params must be [N, 24]')
    if id_lut is not None and id_lut.numel() < 256:
        raise EssHipError('augment_perspective_filter: id_lut must have 256 entries')
    if scratch is None:
        scratch = torch.empty(N, H, W, dtype=torch.float32, device=img.device)
    else:
        _formed('augment_perspective_filter', 'scratch', scratch, torch.float32, (N, H, W))
    if out is None:
        out = torch.empty(N, 1, H, W, dtype=torch.float32, device=img.device)
        out_l = torch.empty(N, H, W, dtype=torch.int64, device=img.device) if label is not None else None
    else:
        if not isinstance(out, (tuple, list)) or len(out) != 2 or (out[1] is None) != (label is None):
            raise EssHipError('augment_perspective_filter: out must be (img, label) with a label tensor exactly where a label is given')
        out, out_l = _formed('augment_perspective_filter', 'out[0]', out[0], torch.float32, (N, 1, H, W)), out[1]
        if out_l is not None:
            _formed('augment_perspective_filter', 'out[1]', out_l, torch.int64, (N, H, W))
    _check(lib().ess_augment_perspective_filter(ptr(img), ptr(label, torch.int64), ptr(params), ptr(id_lut, torch.int64), ptr(scratch),
                                                ptr(out), ptr(out_l, torch.int64), N, H, W, stream()), 'ess_augment_perspective_filter')
    return out, out_l


def radam_step(p, g, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step_size, n_sma_ge5):
    _check(lib().ess_radam_step(ptr(p), ptr(g), ptr(exp_avg), ptr(exp_avg_sq), p.numel(), c_float(lr), c_float(beta1),
                                c_float(beta2), c_float(eps), c_float(step_size), int(n_sma_ge5), stream()),
           'ess_radam_step')


def radam_step_dev(p, g, exp_avg, exp_avg_sq, beta1, beta2, eps, hyper):
    """RAdam update with (-step_size * lr, rectified?) read from the device tensor `hyper` (2 floats)."""
    _check(lib().ess_radam_step_dev(ptr(p), ptr(g), ptr(exp_avg), ptr(exp_avg_sq), p.numel(), c_float(beta1), c_float(beta2),
                                    c_float(eps), ptr(hyper), stream()), 'ess_radam_step_dev')


def resize_nearest(x, size):
    """F.interpolate(x, size=size, mode='nearest') for fp32 NCHW (identity when the size already matches)."""
    N, C, h, w = x.shape
    H, W = int(size[0]), int(size[1])
    if (h, w) == (H, W):
        return x
    y = torch.empty(N, C, H, W, dtype=torch.float32, device=x.device)
    _check(lib().ess_resize_nearest(ptr(x), ptr(y), N * C, h, w, H, W, stream()), 'ess_resize_nearest')
    return y


NORM_SPLIT_BY_PLANE = 1 << 30  # ESS_NORM_SPLIT_BY_PLANE: tuning_set('norm_split_wgs', ...) -- the plane size alone decides the split


def tuning_set(key, value):
    """Process-wide kernel-choice switch (include/ess_hip.h).  'conv_wide': results are identical for every setting;
    'in_small_threads' and 'norm_split_wgs' change the summation order of the norm statistics, i.e. results in their last bits
    ('norm_split_wgs': NORM_SPLIT_BY_PLANE makes that order independent of the batch size; a value <= 0 returns to the process's own
    setting)."""
    _check(lib().ess_tuning_set(key.encode(), int(value)), 'ess_tuning_set')


def tuning_get(key):
    v = c_int32(0)
    _check(lib().ess_tuning_get(key.encode(), byref(v)), 'ess_tuning_get')
    return v.value


def label_confusion(pred, labels, conf, ignore_index=255):
    """conf[label, pred] += 1 over labels != ignore_index, for given int64 predictions (no argmax)."""
    if pred.shape != labels.shape or pred.dtype != torch.int64 or labels.dtype != torch.int64:
        raise EssHipError(f'label_confusion: int64 tensors of one shape expected, got {pred.dtype}{tuple(pred.shape)} / {labels.dtype}{tuple(labels.shape)}')
    if pred.numel():
        _check(lib().ess_label_confusion(ptr(pred, torch.int64), ptr(labels, torch.int64), ptr(conf, torch.int64),
                                         c_int64(pred.numel()), conf.shape[0], int(ignore_index), stream()), 'ess_label_confusion')
    return conf


def argmax_confusion(logits, labels=None, conf=None, ignore_index=255, want_pred=True):
    N, K, H, W = logits.shape
    pred = torch.empty(N, H, W, dtype=torch.int64, device=logits.device) if want_pred else None
    _check(lib().ess_argmax_confusion(ptr(logits), ptr(labels, torch.int64), ptr(pred, torch.int64), ptr(conf, torch.int64),
                                      N, K, H * W, int(ignore_index), stream()), 'ess_argmax_confusion')
    return pred


SEG_HEAD_MAX_K = 64


def _seg_head_args(who, x, C, weight, bias, out_hw, window, palette):
    """the argument checks hip.seg_head and hip.seg_head_eval share -> (fmt, weight [K, C], N, K, H, W, (y0, x0, h, w), (Ho, Wo))"""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise EssHipError(f'{who}: x must be a CUDA(HIP) tensor; there is no CPU path')
    if x.dim() == 5 and x.shape[-1] == 8 and x.dtype in (torch.bfloat16, torch.float16):
        fmt = FMT_F16_C8 if (x.dtype == torch.float16 or is_f16_c8(x)) else FMT_BF16_C8
        N, nb, H, W, _ = x.shape
        if not 0 < C <= nb * 8:
            raise EssHipError(f'{who}: C={C} channels do not fit the source\'s {nb} blocks of 8')
        if nb != (C + 7) // 8:
            raise EssHipError(f'{who}: C={C} channels need {(C + 7) // 8} blocks of 8, x has {nb}')
    elif x.dim() == 4 and x.dtype == torch.float32:
        fmt = FMT_F32_NCHW
        N, Cx, H, W = x.shape
        if Cx != C:
            raise EssHipError(f'{who}: C={C} but x has {Cx} channels')
    else:
        raise EssHipError(f'{who}: x must be fp32 NCHW, BF16_C8 or F16_C8, got {x.dtype}{tuple(x.shape)}')
    if weight.dim() == 4 and weight.shape[2:] == (1, 1):
        weight = weight.view(weight.shape[0], weight.shape[1])
    if weight.dim() != 2 or weight.shape[1] != C:
        raise EssHipError(f'{who}: weight must be [K, C={C}], got {tuple(weight.shape)}')
    K = weight.shape[0]
    if not 0 < K <= SEG_HEAD_MAX_K:
        raise EssHipError(f'{who}: weight has K={K} classes, at most {SEG_HEAD_MAX_K} are supported')
    if bias is None or tuple(bias.shape) != (K,):
        raise EssHipError(f'{who}: bias must be [K={K}], got {None if bias is None else tuple(bias.shape)}')
    if palette is not None and (not torch.is_tensor(palette) or palette.dtype != torch.uint8 or tuple(palette.shape) != (K, 3)):
        got = f'{palette.dtype}{tuple(palette.shape)}' if torch.is_tensor(palette) else type(palette).__name__
        raise EssHipError(f'{who}: palette must be a uint8 [K={K}, 3] tensor, got {got}')
    y0, x0, h, w = (0, 0, H, W) if window is None else (int(v) for v in window)
    if y0 < 0 or x0 < 0 or h <= 0 or w <= 0 or y0 + h > H or x0 + w > W:
        raise EssHipError(f'{who}: window {(y0, x0, h, w)} leaves the {H} x {W} source plane')
    Ho, Wo = (h, w) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    if Ho <= 0 or Wo <= 0:
        raise EssHipError(f'{who}: out_hw {(Ho, Wo)} is empty')
    return fmt, weight, N, K, H, W, (y0, x0, h, w), (Ho, Wo)


def _seg_head_outputs(N, Ho, Wo, palette, want_confidence, dev):
    labels = torch.empty(N, Ho, Wo, dtype=torch.uint8, device=dev)
    colour = torch.empty(N, Ho, Wo, 3, dtype=torch.uint8, device=dev) if palette is not None else None
    conf = torch.empty(N, Ho, Wo, dtype=torch.float32, device=dev) if want_confidence else None
    return labels, colour, conf


def seg_head(x, C, weight, bias, out_hw=None, window=None, palette=None, want_confidence=False):
    """Fused class head at inference (ess_seg_head): labels = first argmax_k (bias[k] + sum_c weight[k, c] x[c]) per output pixel,
    without the scores ever being written -> (labels uint8 [N, H_out, W_out], colour uint8 [N, H_out, W_out, 3] or None, confidence
    fp32 [N, H_out, W_out] or None).
    x: the activation in front of the 1x1 class convolution, C channels: fp32 NCHW, BF16_C8, or F16_C8 (a float16 tensor
    [N, C/8, H, W, 8], or the bfloat16-typed container of f16_c8_empty); weight [K, C] (or the convolution's [K, C, 1, 1]) and bias
    [K]: the plain fp32 parameters -- the kernel rounds the weight to the source's operand type itself.
    window (y0, x0, h, w): the part of the source plane the output is taken from (default: all of it); out_hw: the output size
    (default: the window's) -- source pixels by hip.resize_nearest's index rule inside the window, so labels equal
    argmax(resize_nearest(scores)).  palette: uint8 [K, 3] on the device -> colour = palette[labels].  want_confidence: the softmax
    probability of the winning class."""
    fmt, weight, N, K, H, W, (y0, x0, h, w), (Ho, Wo) = _seg_head_args('seg_head', x, C, weight, bias, out_hw, window, palette)
    labels, colour, conf = _seg_head_outputs(N, Ho, Wo, palette, want_confidence, x.device)
    _check(lib().ess_seg_head(ptr(x, x.dtype, allow_none=False), fmt, ptr(weight.detach(), allow_none=False), ptr(bias.detach(), allow_none=False),
                              ptr(palette, torch.uint8), ptr(labels, torch.uint8), ptr(colour, torch.uint8), ptr(conf), N, C, K, H, W,
                              y0, x0, h, w, Ho, Wo, stream()), 'ess_seg_head')
    return labels, colour, conf


def seg_head_eval(x, C, weight, bias, gt, confusion, ignore_index=255, out_hw=None, window=None, palette=None, want_confidence=False):
    """hip.seg_head that scores itself (ess_seg_head_eval): the same (labels, colour, confidence), bit for bit, and per sample
    confusion[n, gt, label] += 1 over the output pixels with gt != ignore_index and gt < K.  gt: uint8 [N, H_out, W_out]; confusion:
    int64 [N, K, K], both contiguous on the device; confusion is ADDED to (integer sums: order-independent), never zeroed."""
    fmt, weight, N, K, H, W, (y0, x0, h, w), (Ho, Wo) = _seg_head_args('seg_head_eval', x, C, weight, bias, out_hw, window, palette)
    if gt is None or confusion is None:
        raise EssHipError('seg_head_eval: gt and confusion come together (hip.seg_head is the head without scoring)')
    for name, t, dtype, shape in (('gt', gt, torch.uint8, (N, Ho, Wo)), ('confusion', confusion, torch.int64, (N, K, K))):
        if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
            got = f'{t.dtype}{tuple(t.shape)}' if torch.is_tensor(t) else type(t).__name__
            raise EssHipError(f'seg_head_eval: {name} must be a contiguous {dtype} {list(shape)} tensor on the device, got {got}')
    labels, colour, conf = _seg_head_outputs(N, Ho, Wo, palette, want_confidence, x.device)
    _check(lib().ess_seg_head_eval(ptr(x, x.dtype, allow_none=False), fmt, ptr(weight.detach(), allow_none=False),
                                   ptr(bias.detach(), allow_none=False), ptr(palette, torch.uint8), ptr(labels, torch.uint8),
                                   ptr(colour, torch.uint8), ptr(conf), ptr(gt, torch.uint8), ptr(confusion, torch.int64),
                                   int(ignore_index), N, C, K, H, W, y0, x0, h, w, Ho, Wo, stream()), 'ess_seg_head_eval')
    return labels, colour, conf


# ------------------------------------------------------------------------------------------ reconstruction post-processing
RECON_POST_PARTIALS = 256   # ESS_RECON_POST_PARTIALS: min / max partial pairs per sample in recon_post_bounds' workspace
RECON_POST_MAX_FILTER = 63  # ESS_RECON_POST_MAX_FILTER: the largest auto_hdr_median_filter_size (a history of 64 entries: one wave)
PREVIEW_MODES = {'red-blue': 0, 'grayscale': 1}  # ESS_PREVIEW_RED_BLUE, ESS_PREVIEW_GRAYSCALE


def _formed(fn, name, t, dtype, shape):
    """`t` is a contiguous `dtype` tensor of `shape`, or the call is refused (where it lies is _on_device's question, asked last)"""
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        got = f'{t.dtype}{tuple(t.shape)}' if torch.is_tensor(t) else type(t).__name__
        raise EssHipError(f'{fn}: {name} must be a contiguous {dtype} {list(shape)} tensor, got {got}')
    return t


def _recon_post_image(fn, img, weights, amount):
    """-> (N, Hs, Ws, the 25 weights as a ctypes array or None, c1, amount)"""
    if not torch.is_tensor(img) or img.dtype != torch.float32 or img.dim() != 4 or img.shape[1] != 1 or img.numel() == 0 or not img.is_contiguous():
        got = f'{img.dtype}{tuple(img.shape)}' if torch.is_tensor(img) else type(img).__name__
        raise EssHipError(f'{fn}: img must be a non-empty contiguous fp32 [N, 1, Hs, Ws] tensor, got {got}')
    amount = float(amount)
    if amount != amount:
        raise EssHipError(f'{fn}: amount is NaN')
    w = None
    if amount > 0:
        if weights is None:
            raise EssHipError(f'{fn}: amount={amount} > 0 needs the 5 x 5 weights')
        flat = np.asarray(weights.detach().cpu() if torch.is_tensor(weights) else weights, dtype=np.float32).reshape(-1)
        if flat.size != 25 or not np.isfinite(flat).all():
            raise EssHipError(f'{fn}: weights must be 25 finite values (5 x 5), got {flat.size}')
        w = (c_float * 25)(*flat.tolist())
    c1 = float(np.float32(1 + amount))  # (1 + amount) in double, rounded to fp32 once: the reference's `(1 + amount) * img`
    return img.shape[0], img.shape[2], img.shape[3], w, c1, float(np.float32(amount))


def _steer_words(fn, name, t, N):
    """a steering table of a steered recon_post call: int32 [N], contiguous (its memory is _on_device's question)"""
    if not torch.is_tensor(t) or t.dtype != torch.int32 or tuple(t.shape) != (N,) or not t.is_contiguous():
        got = f'{t.dtype}{tuple(t.shape)}' if torch.is_tensor(t) else type(t).__name__
        raise EssHipError(f'{fn}: {name} must be a contiguous int32 [{N}] tensor (one word per slot), got {got}')
    return t


def recon_post_frame(img, weights, amount, bounds, window=None, out_u8=None, out_f32=None, want_u8=True, want_f32=False, mode=None):
    """Unsharp mask + intensity rescale + 8-bit quantisation in one pass (ess_recon_post_frame) -> (frame_u8 [N, H, W] uint8 or None,
    frame_f32 [N, 1, H, W] = float(u8) / 255 or None).  img: fp32 [N, 1, Hs, Ws]; weights: the 5 x 5 Gaussian (host values; unused for
    amount <= 0, which skips the stencil); bounds: fp32 [N, 2] ON THE DEVICE = (Imin, Imax - Imin) per sample; window (y0, x0, H, W): the
    part of the source that is written (default: all) -- the stencil still sees the whole source, zero beyond its borders.  out_u8 /
    out_f32: the caller's output tensors.  Per pixel, in fp32 without fused operations: blur = sum of w * v in row-major tap order,
    s = c1 v - amount blur, q = (255 (s - Imin)) / range, clamped to [0, 255] and truncated.  A NaN pixel gives 0.
    mode (default None: the call above, launch for launch): int32 [N] ON THE DEVICE, one word per slot (ess_recon_post_frame_steered): a
    slot whose word is neither CARRY_TAKE nor CARRY_ZERO is neither read nor written -- its rows of out_u8 / out_f32 keep what they
    held (of a tensor allocated here: unspecified) --, every other slot gets the unsteered call's bits."""
    fn = 'recon_post_frame'
    N, Hs, Ws, w, c1, amount = _recon_post_image(fn, img, weights, amount)
    y0, x0, H, W = (0, 0, Hs, Ws) if window is None else (int(v) for v in window)
    if y0 < 0 or x0 < 0 or H <= 0 or W <= 0 or y0 + H > Hs or x0 + W > Ws:
        raise EssHipError(f'{fn}: window {(y0, x0, H, W)} leaves the {Hs} x {Ws} source')
    if out_u8 is None and out_f32 is None and not want_u8 and not want_f32:
        raise EssHipError(f'{fn}: neither frame_u8 nor frame_f32 is asked for')
    _formed(fn, 'bounds', bounds, torch.float32, (N, 2))
    if out_u8 is not None:
        _formed(fn, 'out_u8', out_u8, torch.uint8, (N, H, W))
    if out_f32 is not None:
        _formed(fn, 'out_f32', out_f32, torch.float32, (N, 1, H, W))
    if mode is not None:
        _steer_words(fn, 'mode', mode, N)
    _on_device(fn, [(k, v) for k, v in (('mode', mode), ('img', img), ('bounds', bounds), ('out_u8', out_u8), ('out_f32', out_f32))
                    if v is not None])
    if out_u8 is None and want_u8:
        out_u8 = torch.empty(N, H, W, dtype=torch.uint8, device=img.device)
    if out_f32 is None and want_f32:
        out_f32 = torch.empty(N, 1, H, W, dtype=torch.float32, device=img.device)
    if mode is not None:
        _check(lib().ess_recon_post_frame_steered(ptr(img), w, c1, amount, ptr(bounds), ptr(out_u8, torch.uint8), ptr(out_f32), N, Hs, Ws,
                                                  y0, x0, H, W, ptr(mode, torch.int32), stream()), 'ess_recon_post_frame_steered')
        return out_u8, out_f32
    _check(lib().ess_recon_post_frame(ptr(img), w, c1, amount, ptr(bounds), ptr(out_u8, torch.uint8), ptr(out_f32), N, Hs, Ws, y0, x0, H, W,
                                      stream()), 'ess_recon_post_frame')
    return out_u8, out_f32


def recon_post_bounds(img, weights, amount, workspace, ring, ring_state, filter_size, bounds, mode=None, rows=None):
    """The auto-HDR step of IntensityRescaler with its history on the device (ess_recon_post_bounds; two launches, no
    synchronisation): min / max of the SHARPENED source per sample -> clip to [0, 0.45] / [0.55, 1] in fp64 -> push into the sample's
    history (ring fp64 [N, filter_size + 1, 2], ring_state int32 [N, 2] = (head, count); zeros = empty) -> bounds[n] = (median of the
    held mins, median of the held maxs minus it), np.median's rule.  workspace: fp32 [N, RECON_POST_PARTIALS, 2], fully rewritten.
    Deviation: NaN pixels are skipped by the min / max (torch.min / max would hand NaN on).
    mode / rows (default None, None: the call above, launch for launch; rows needs mode): the step STEERED per slot
    (ess_recon_post_bounds_steered).  img then holds N SLOTS, workspace [N, PARTIALS, 2] and bounds [N, 2] are indexed by slot, ring
    [R, filter_size + 1, 2] and ring_state [R, 2] hold R history ROWS (without rows: R == N and slot n's row is n).  mode: int32 [N] ON
    THE DEVICE -- CARRY_TAKE: the step above on the slot's row; CARRY_ZERO: the same from an EMPTIED history (the restart);
    CARRY_HOLD, any other word, or a row outside [0, R): the slot is skipped -- no image read, its workspace, bounds and every history
    untouched.  rows: int32 [N] on the device, or a host list of N ints (checked here: two slots naming one row are refused; then
    uploaded, which a capture cannot record -- a captured caller hands a device tensor whose rows are distinct by construction)."""
    fn = 'recon_post_bounds'
    N, Hs, Ws, w, c1, amount = _recon_post_image(fn, img, weights, amount)
    if rows is not None and mode is None:
        raise EssHipError(f'{fn}: rows= belongs to the steered step: pass mode= (int32 [{N}] on the device) with it')
    R = N
    if mode is not None:
        _steer_words(fn, 'mode', mode, N)
        if not torch.is_tensor(ring_state) or ring_state.dim() != 2 or ring_state.shape[0] < 1:
            got = f'{ring_state.dtype}{tuple(ring_state.shape)}' if torch.is_tensor(ring_state) else type(ring_state).__name__
            raise EssHipError(f'{fn}: ring_state must be an int32 [R, 2] tensor of R >= 1 history rows, got {got}')
        if rows is not None:
            R = ring_state.shape[0]
            if not torch.is_tensor(rows):
                if isinstance(rows, (str, bytes)) or not hasattr(rows, '__len__') or len(rows) != N or \
                        any(isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not -2 ** 31 <= r < 2 ** 31 for r in rows):
                    raise EssHipError(f'{fn}: rows must be an int32 [{N}] device tensor or a host list of {N} ints, got {rows!r}')
                named = [int(r) for r in rows if 0 <= r < R]
                if len(set(named)) != len(named):
                    raise EssHipError(f'{fn}: rows={list(rows)} names a history row twice: one call takes one frame per row')
            else:
                _steer_words(fn, 'rows', rows, N)
    if isinstance(filter_size, bool) or int(filter_size) != filter_size or not 0 <= filter_size <= RECON_POST_MAX_FILTER:
        raise EssHipError(f'{fn}: filter_size={filter_size} outside 0..{RECON_POST_MAX_FILTER}')
    filter_size = int(filter_size)
    if N > 65535:
        raise EssHipError(f'{fn}: N={N} samples, at most 65535')
    for name, t, dtype, shape in (('workspace', workspace, torch.float32, (N, RECON_POST_PARTIALS, 2)),
                                  ('ring', ring, torch.float64, (R, filter_size + 1, 2)),
                                  ('ring_state', ring_state, torch.int32, (R, 2)), ('bounds', bounds, torch.float32, (N, 2))):
        _formed(fn, name, t, dtype, shape)
    steer = [(k, v) for k, v in (('mode', mode), ('rows', rows)) if torch.is_tensor(v)]
    _on_device(fn, steer + [('img', img), ('workspace', workspace), ('ring', ring), ('ring_state', ring_state), ('bounds', bounds)])
    if mode is not None:
        if rows is not None and not torch.is_tensor(rows):
            rows = torch.tensor([int(r) for r in rows], dtype=torch.int32).to(img.device)
        _check(lib().ess_recon_post_bounds_steered(ptr(img), w, c1, amount, N, Hs, Ws, ptr(workspace), c_size_t(workspace.numel() * 4),
                                                   ptr(ring, torch.float64), ptr(ring_state, torch.int32), R, filter_size, ptr(bounds),
                                                   ptr(mode, torch.int32), ptr(rows, torch.int32), stream()),
               'ess_recon_post_bounds_steered')
        return bounds
    _check(lib().ess_recon_post_bounds(ptr(img), w, c1, amount, N, Hs, Ws, ptr(workspace), c_size_t(workspace.numel() * 4),
                                       ptr(ring, torch.float64), ptr(ring_state, torch.int32), filter_size, ptr(bounds), stream()),
           'ess_recon_post_bounds')
    return bounds


def event_preview(grids, mode='red-blue', num_bins_to_show=-1, out=None):
    """make_event_preview for every sample of fp32 [N, C, H, W] grids (ess_event_preview) -> uint8 [N, H, W, 3] in BGR order
    ('red-blue': blue 255 where the bin sum is > 0, red 255 where it is < 0) or uint8 [N, H, W] ('grayscale': 255 (s + 10) / 20).
    The last num_bins_to_show planes are summed in plane order (< 0: all).  Deviation: the grey value is clamped to [0, 255] BEFORE the
    cast; the reference casts first and lets values outside the range wrap."""
    fn = 'event_preview'
    if mode not in PREVIEW_MODES:
        raise EssHipError(f"{fn}: mode must be 'red-blue' or 'grayscale', got {mode!r}")
    if not torch.is_tensor(grids) or grids.dtype != torch.float32 or grids.dim() != 4 or grids.numel() == 0 or not grids.is_contiguous():
        got = f'{grids.dtype}{tuple(grids.shape)}' if torch.is_tensor(grids) else type(grids).__name__
        raise EssHipError(f'{fn}: grids must be a non-empty contiguous fp32 [N, C, H, W] tensor, got {got}')
    if isinstance(num_bins_to_show, bool) or int(num_bins_to_show) != num_bins_to_show:
        raise EssHipError(f'{fn}: num_bins_to_show={num_bins_to_show!r} is no whole number')
    N, C, H, W = grids.shape
    shape = (N, H, W, 3) if mode == 'red-blue' else (N, H, W)
    if out is not None:
        _formed(fn, 'out', out, torch.uint8, shape)
    _on_device(fn, [('grids', grids)] + ([('out', out)] if out is not None else []))
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=grids.device)
    _check(lib().ess_event_preview(ptr(grids), ptr(out, torch.uint8), N, C, H, W, max(-1, min(int(num_bins_to_show), C)), PREVIEW_MODES[mode], stream()),
           'ess_event_preview')
    return out


# ------------------------------------------------------------------------------------------ segmentation display
VIZ_EVENT_MODES = {'histogram': 0, 'separate_pol': 1, 'signed': 2}  # ESS_VIZ_HISTOGRAM, ESS_VIZ_SEPARATE_POL, ESS_VIZ_SIGNED
GRID_PADDING = 2  # make_grid's default


def grid_geometry(n, H, W, nrow=8, padding=GRID_PADDING):
    """make_grid's layout of n tiles of H x W -> (xmaps, ymaps, Hg, Wg): xmaps = min(nrow, n) tiles per grid row, ymaps = ceil(n / xmaps)
    grid rows; tile k at rows (k // xmaps) (H + padding) + padding, columns (k % xmaps) (W + padding) + padding."""
    xmaps = min(int(nrow), n)
    ymaps = -(-n // xmaps)
    return xmaps, ymaps, ymaps * (H + padding) + padding, xmaps * (W + padding) + padding


def _viz_dst(fn, out, dst, N, H, W, ref):
    """where a tile writer writes -> (the tensor returned, pointer, elements owned from it on, EssVizDst).  out: a contiguous fp32
    [N, 3, H, W] tensor (None: a new one); dst = (panel fp32 [3, Hg, Wg], tile0, xmaps, padding): the N tiles go to slots tile0 ..
    tile0 + N - 1 of the panel's grid."""
    if dst is not None:
        if out is not None:
            raise EssHipError(f'{fn}: out and dst exclude each other')
        panel, tile0, xmaps, padding = dst
        tile0, xmaps, padding = int(tile0), int(xmaps), int(padding)
        if not torch.is_tensor(panel) or panel.dtype != torch.float32 or panel.dim() != 3 or panel.shape[0] != 3 or not panel.is_contiguous():
            got = f'{panel.dtype}{tuple(panel.shape)}' if torch.is_tensor(panel) else type(panel).__name__
            raise EssHipError(f'{fn}: the panel must be a contiguous fp32 [3, Hg, Wg] tensor, got {got}')
        Hg, Wg = panel.shape[1:]
        if tile0 < 0 or xmaps < 1 or padding < 0 or xmaps * (W + padding) + padding > Wg or \
                ((tile0 + N - 1) // xmaps + 1) * (H + padding) + padding > Hg:
            raise EssHipError(f'{fn}: tiles {tile0}..{tile0 + N - 1} of {H} x {W} ({xmaps} per row, padding {padding}) leave the {Hg} x {Wg} panel')
        _on_device(fn, [('panel', panel), ref])
        off = padding * Wg + padding
        d = EssVizDst(Hg * Wg, Wg, (H + padding) * Wg, W + padding, tile0, xmaps)
        return panel, c_void_p(panel.data_ptr() + 4 * off), c_size_t(panel.numel() - off), d
    if out is not None:
        _formed(fn, 'out', out, torch.float32, (N, 3, H, W))
    _on_device(fn, [ref] + ([('out', out)] if out is not None else []))
    if out is None:
        out = torch.empty(N, 3, H, W, dtype=torch.float32, device=ref[1].device)
    return out, c_void_p(out.data_ptr()), c_size_t(out.numel()), EssVizDst(H * W, W, 3 * H * W, 0, 0, 1)


_colour_tables = {}


def viz_colour_table(color_map, device):
    """prepare_semseg's colour table: fp32 [K, 3] on `device`, divided by 255 (in fp32) if its maximum exceeds 128.  A host colour map
    (list / numpy) is scaled on the host and uploaded once per content; a device tensor is scaled without a synchronisation."""
    if torch.is_tensor(color_map) and color_map.is_cuda:
        c = color_map.to(torch.float32)
        if c.dim() != 2 or c.shape[1] != 3 or c.shape[0] == 0:
            raise EssHipError(f'viz_colour_table: the colour map must be [K, 3], got {tuple(c.shape)}')
        # (tensor / tensor: a division by a Python scalar is a multiplication with its reciprocal on the device, another last bit)
        return torch.where(c.max() > 128, c / torch.full_like(c, 255), c).contiguous()
    c = np.ascontiguousarray(np.asarray(color_map.cpu() if torch.is_tensor(color_map) else color_map, dtype=np.float32))
    if c.ndim != 2 or c.shape[1] != 3 or c.shape[0] == 0:
        raise EssHipError(f'viz_colour_table: the colour map must be [K, 3], got {c.shape}')
    key = (c.tobytes(), c.shape[0], str(device))
    t = _colour_tables.get(key)
    if t is None:
        if c.max() > 128:
            c = c / np.float32(255)
        if len(_colour_tables) >= 16:
            _colour_tables.clear()
        t = _colour_tables[key] = torch.from_numpy(c).to(device)
    return t


def viz_semseg(labels, colours, ignore_label=255, out=None, dst=None):
    """prepare_semseg on the device (ess_viz_semseg): labels uint8 or int64 [N, H, W] + colours fp32 [K, 3] on the 0..1 scale
    (viz_colour_table) -> fp32 [N, 3, H, W] (out, or a new tensor), or the N tiles written into their slots of a panel (dst = (panel,
    tile0, xmaps, padding), see grid_geometry).  The ignore label shows create_checkerboard's pattern.  Deviation: so does any other
    label outside [0, K), where the reference asserts on the host."""
    fn = 'viz_semseg'
    if not torch.is_tensor(labels) or labels.dtype not in (torch.uint8, torch.int64) or labels.dim() != 3 or labels.numel() == 0 \
            or not labels.is_contiguous():
        got = f'{labels.dtype}{tuple(labels.shape)}' if torch.is_tensor(labels) else type(labels).__name__
        raise EssHipError(f'{fn}: labels must be a non-empty contiguous uint8 or int64 [N, H, W] tensor, got {got}')
    if not torch.is_tensor(colours) or colours.dtype != torch.float32 or colours.dim() != 2 or colours.shape[1] != 3 or colours.shape[0] == 0 \
            or not colours.is_contiguous():
        got = f'{colours.dtype}{tuple(colours.shape)}' if torch.is_tensor(colours) else type(colours).__name__
        raise EssHipError(f'{fn}: colours must be a contiguous fp32 [K, 3] tensor, got {got}')
    if isinstance(ignore_label, bool) or int(ignore_label) != ignore_label or not -2 ** 31 <= ignore_label < 2 ** 31:
        raise EssHipError(f'{fn}: ignore_label={ignore_label!r} is no 32-bit whole number')
    N, H, W = labels.shape
    ret, p_out, elems, d = _viz_dst(fn, out, dst, N, H, W, ('labels', labels))
    _on_device(fn, [('colours', colours)])
    _check(lib().ess_viz_semseg(c_void_p(labels.data_ptr()), 0 if labels.dtype == torch.uint8 else 1, ptr(colours), p_out, elems,
                                ctypes.byref(d), N, colours.shape[0], H, W, int(ignore_label), stream()), 'ess_viz_semseg')
    return ret


def viz_events(x, mode, unit=False, out=None, dst=None):
    """An event tensor's RGB tile (ess_viz_events): x fp32 [N, C, H, W] -> fp32 [N, 3, H, W] or panel slots (dst, as viz_semseg).
    'histogram' (C = 2): (clamp(x0), clamp(x1), 0).  'separate_pol' (C even, >= 4): (clamp(neg), clamp(pos), 0) with pos / neg the
    sums over a polarity's half of x[c] * ((c + 1) / half), ascending c, fp32.  'signed' (C > 3): 255 -- 1 with unit=True -- in plane 0
    where the channel sum is > 0 and in plane 2 where it is < 0."""
    fn = 'viz_events'
    if mode not in VIZ_EVENT_MODES:
        raise EssHipError(f"{fn}: mode must be 'histogram', 'separate_pol' or 'signed', got {mode!r}")
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 4 or x.numel() == 0 or not x.is_contiguous():
        got = f'{x.dtype}{tuple(x.shape)}' if torch.is_tensor(x) else type(x).__name__
        raise EssHipError(f'{fn}: x must be a non-empty contiguous fp32 [N, C, H, W] tensor, got {got}')
    N, C, H, W = x.shape
    if mode == 'histogram' and C != 2:
        raise EssHipError(f'{fn}: the histogram tile needs C = 2 channels, got {C}')
    if mode == 'separate_pol' and (C < 4 or C % 2):
        raise EssHipError(f'{fn}: the separate_pol tile needs an even C >= 4 (a polarity per half), got {C}')
    if mode == 'signed' and C <= 3:
        raise EssHipError(f'{fn}: the signed tile needs C > 3 channels, got {C}')
    ret, p_out, elems, d = _viz_dst(fn, out, dst, N, H, W, ('x', x))
    _check(lib().ess_viz_events(ptr(x), p_out, elems, ctypes.byref(d), N, C, H, W, VIZ_EVENT_MODES[mode], int(bool(unit)), stream()),
           'ess_viz_events')
    return ret


def viz_overlay(labels, gray, palette, alpha, out=None):
    """Label colours over a gray frame (ess_viz_overlay): labels, gray uint8 [N, H, W]; palette uint8 [K, 3]; 0 <= alpha <= 1 ->
    uint8 [N, H, W, 3] = (uint8) min((1 - alpha) gray + alpha palette[label] + 0.5, 255) in fp32 (two products, one sum; the palette's
    channel order).  A label >= K shows the gray value.  The arithmetic is this package's own, not the reference's."""
    fn = 'viz_overlay'
    for name, t in (('labels', labels), ('gray', gray)):
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 3 or t.numel() == 0 or not t.is_contiguous():
            got = f'{t.dtype}{tuple(t.shape)}' if torch.is_tensor(t) else type(t).__name__
            raise EssHipError(f'{fn}: {name} must be a non-empty contiguous uint8 [N, H, W] tensor, got {got}')
    if tuple(labels.shape) != tuple(gray.shape):
        raise EssHipError(f'{fn}: labels {tuple(labels.shape)} and the frame {tuple(gray.shape)} differ in size')
    if not torch.is_tensor(palette) or palette.dtype != torch.uint8 or palette.dim() != 2 or palette.shape[1] != 3 \
            or not 1 <= palette.shape[0] <= 256 or not palette.is_contiguous():
        got = f'{palette.dtype}{tuple(palette.shape)}' if torch.is_tensor(palette) else type(palette).__name__
        raise EssHipError(f'{fn}: palette must be a contiguous uint8 [K, 3] tensor with K <= 256, got {got}')
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise EssHipError(f'{fn}: alpha={alpha} outside [0, 1]')
    N, H, W = labels.shape
    if out is not None:
        _formed(fn, 'out', out, torch.uint8, (N, H, W, 3))
    _on_device(fn, [('labels', labels), ('gray', gray), ('palette', palette)] + ([('out', out)] if out is not None else []))
    if out is None:
        out = torch.empty(N, H, W, 3, dtype=torch.uint8, device=labels.device)
    _check(lib().ess_viz_overlay(ptr(labels, torch.uint8), ptr(gray, torch.uint8), ptr(palette, torch.uint8), ptr(out, torch.uint8), N,
                                 palette.shape[0], H, W, alpha, stream()), 'ess_viz_overlay')
    return out


# ------------------------------------------------------------------------------------------ 'mixed' configuration (ESS_COMPUTE_F16)
def f16_blocks_empty(N, C, H, W, device, hilo=False):
    """Uninitialised F16_C8 tensor of a logical [N, C, H, W] activation: float16 [N][ceil(C/8)][H][W][8]; hilo: the [hi | lo] pair
    [N][2 ceil(C/8)][H][W][8] (ESS_FMT_F16_C8_HILO)."""
    return torch.empty(N, ((C + 7) // 8) * (2 if hilo else 1), H, W, 8, dtype=torch.float16, device=device)


def h16_of(t):
    return copies.of(t).h16  # ((half copy, hilo) or None, under its earlier name: the GPU tests read it)


def attach_h16(t, h16, hilo=False):
    return copies.attach(t, h16=(h16, bool(hilo)))


def to_f16_c8(x, hilo=False):
    """fp32 NCHW -> F16_C8 (hilo: the [hi | lo] pair) on the device."""
    N, C, H, W = x.shape
    y = f16_blocks_empty(N, C, H, W, x.device, hilo)
    _check(lib().ess_to_f16_c8(ptr(x), ptr(y, torch.float16), N, C, H, W, int(bool(hilo)), stream()), 'ess_to_f16_c8')
    return y


def bf16_c8_to_f16_c8(x):
    """BF16_C8 -> F16_C8 (exact inside half's range)."""
    y = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    _check(lib().ess_bf16_c8_to_f16_c8(ptr(x, torch.bfloat16), ptr(y, torch.float16), x.numel() // 8, stream()), 'ess_bf16_c8_to_f16_c8')
    return y


def f16_c8_to_bf16_c8(x, hilo=False):
    """F16_C8 (or, hilo, a [hi | lo] pair: hi + lo) -> BF16_C8, round to nearest even."""
    N, nb, H, W, _ = x.shape
    CB = nb // 2 if hilo else nb
    y = torch.empty(N, CB, H, W, 8, dtype=torch.bfloat16, device=x.device)
    _check(lib().ess_f16_c8_to_bf16_c8(ptr(x, torch.float16), ptr(y, torch.bfloat16), N, CB * 8, H, W, int(bool(hilo)), stream()),
           'ess_f16_c8_to_bf16_c8')
    return y


def conv_forward_h16(spec, src0, src1, packed_w, scale=None, shift=None, residual=None, aux0=None, aux1=None, out=None, out2=None,
                     out_h16=None, out_fmt=FMT_F32_NCHW, aux_fmt=FMT_F32_NCHW, src_fp32=False):
    """ess_conv2d_forward of an ESS_COMPUTE_F16 spec: src0 / src1 / residual are F16_C8 tensors (float16 [N][C/8][H][W][8]; src_fp32:
    the fp32 NCHW image of the 5x5 head), out_fmt FMT_F16_C8 / FMT_F16_C8_HILO: `out` is a float16 tensor from f16_blocks_empty;
    FMT_F32_NCHW: fp32 (+ out_h16, the half copy); LSTM / GRU: out_fmt / aux_fmt describe the fp32 states, out_h16 the half copy."""
    if spec.desc.compute != COMPUTE_F16:
        raise EssHipError('conv_forward_h16: the spec was not created with compute=COMPUTE_F16')
    sdt = torch.float32 if src_fp32 else torch.float16
    sfmt = FMT_F32_NCHW if src_fp32 else FMT_F16_C8
    half_out = out_fmt in (FMT_F16_C8, FMT_F16_C8_HILO)
    odt = torch.float16 if half_out else torch.float32
    res_fmt = aux_fmt if aux_fmt != FMT_F32_NCHW else ((FMT_F16_C8 if half_out else out_fmt) if residual is not None else FMT_F32_NCHW)
    desc = spec.desc_fmt(sfmt, out_fmt, res_fmt)
    u16 = (spec.desc.act & 1) == GRU_U_F16 and spec.desc.epilogue in (EPI_GRU_UR, EPI_GRU_OUT)
    udt_out = torch.float16 if (u16 and spec.desc.epilogue == EPI_GRU_UR and out_fmt == FMT_F32_C8) else odt
    udt_aux = torch.float16 if (u16 and spec.desc.epilogue == EPI_GRU_OUT and res_fmt == FMT_F32_C8) else torch.float32
    _check(lib().ess_conv2d_forward(byref(desc), ptr(src0, sdt), ptr(src1, sdt), ptr(packed_w, torch.uint8), ptr(scale), ptr(shift),
                                    ptr(residual, torch.float16 if half_out else torch.float32), ptr(aux0), ptr(aux1, udt_aux),
                                    ptr(out, udt_out), ptr(out2, odt), ptr(out_h16, torch.float16), stream()), 'ess_conv2d_forward(f16)')
    return out


def instnorm_forward_c8_mixed(x, C, residual, relu, eps=1e-5, x_fmt=1, want_bf16=True):
    """InstanceNorm of the mixed configuration -> (y BF16_C8 or None, y16 F16_C8, stats).  x: the pre-norm tensor (x_fmt 0 BF16_C8,
    1 F16_C8, 2 the [hi | lo] pair [N][2 CB][H][W][8]) in a bfloat16- or float16-typed container; residual: BF16_C8 (bfloat16) or
    F16_C8 (float16) by its dtype."""
    N, nb, H, W, _ = x.shape
    CB = nb // 2 if x_fmt == 2 else nb
    y = torch.empty(N, CB, H, W, 8, dtype=torch.bfloat16, device=x.device) if want_bf16 else None
    y16 = torch.empty(N, CB, H, W, 8, dtype=torch.float16, device=x.device)
    stats = torch.empty(N * C, 2, dtype=torch.float32, device=x.device)
    L = lib()
    ws = workspace(L.ess_norm_workspace_c8(N * CB), x.device, 'norm8')
    res_f16 = 0
    if residual is not None and residual.dtype == torch.float16:
        res_f16 = 2 if residual.shape[1] == 2 * CB else 1  # (a [hi | lo] pair: twice the blocks; the kernel adds its hi parts)
    _check(L.ess_instnorm_forward_c8_mixed(ptr(x, x.dtype), ptr(residual, residual.dtype if residual is not None else torch.float16),
                                           ptr(y, torch.bfloat16), ptr(y16, torch.float16), ptr(stats), N, C, H * W, c_float(eps),
                                           int(relu), int(x_fmt), int(res_f16), c_void_p(ws.data_ptr()), c_size_t(ws.numel()), stream()),
           'ess_instnorm_forward_c8_mixed')
    return y, y16, stats
