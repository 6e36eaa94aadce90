"""ctypes binding of the C-ABI in include/snnhip.h (libsnnhip.so).

This is host-side plumbing only: every operator call goes through the C entry points, exactly what a cgo/JNI/C++
caller would bind.  The library is mandatory -- there is no CPU or torch fallback; a missing or broken library raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SNNHIP_LIB_PATH") or os.path.join(_HERE, "lib", "libsnnhip.so")  # the override serves ablation builds (tools/)

OK, E_INVALID, E_HIP, E_UNSUPPORTED, E_NOMEM, E_GUARD = 0, -1, -2, -3, -4, -5

ACT = {"": 0, "linear": 0, "none": 0, "relu": 1, "relu6": 2, "tanh": 3, "sigmoid": 4, "leakyRelu": 5, "SiLU": 6, "SiLU_quirk": 7}
PAD_MODE = {"none": 0, "constant": 1, "replicate": 2, "reflect": 3}
DENSE_ACT = {"identity": 0, "": 0, "relu": 1, "leakyRelu": 2, "sigmoid": 3, "softmax": 4, "tanh": 5, "SiLU": 6}


class SnnHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("snnhip error %d: %s" % (code, msg))
        self.code = code


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("N", "H", "W", "IC", "OC", "kh", "kw", "sh", "sw", "padT", "padB", "padL", "padR", "padMode", "act")] + [
        ("leaky", C.c_float), ("useBias", C.c_int), ("useBN", C.c_int), ("dtype", C.c_int), ("OH", C.c_int), ("OW", C.c_int)]


class DenseDesc(C.Structure):
    _fields_ = [("batch", C.c_int), ("in_units", C.c_int), ("out_units", C.c_int), ("act", C.c_int), ("leaky", C.c_float), ("useBias", C.c_int)]


class SubpixelDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("N", "H", "W", "C", "factor", "mode")]


class EltwiseDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("act", C.c_int), ("leaky", C.c_float)]


class Pool2dDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("N", "H", "W", "C", "kh", "kw", "sh", "sw", "padT", "padL", "OH", "OW", "same", "type")]


class PadDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("N", "H", "W", "C", "padT", "padB", "padL", "padR", "mode")]


class UpsampleDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("scale", C.c_float), ("mode", C.c_int)]


class InstanceNormDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("act", C.c_int), ("leaky", C.c_float), ("eps", C.c_float)]


class ConcatDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C0", C.c_int), ("C1", C.c_int), ("OC", C.c_int)]


class UnaryDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("op", C.c_int), ("value", C.c_float)]


class CalculateDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("OC", C.c_int)]


class ResizeDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("OH", C.c_int), ("OW", C.c_int), ("means", C.c_float * 4),
                ("norms", C.c_float * 4), ("linear", C.c_int)]


class ImageU8Desc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("src_channels", C.c_int), ("means", C.c_float * 4), ("norms", C.c_float * 4)]


class U8InDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("dtype", C.c_int), ("means", C.c_float * 4), ("norms", C.c_float * 4)]


class U8OutDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("dtype", C.c_int), ("scale", C.c_float * 4), ("offset", C.c_float * 4)]


class U16InDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("dtype", C.c_int), ("means", C.c_float * 4), ("norms", C.c_float * 4), ("shift", C.c_int)]


class U16OutDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("dtype", C.c_int), ("scale", C.c_float * 4), ("offset", C.c_float * 4), ("maxval", C.c_int),
                ("shift", C.c_int)]


class RgbLumaDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("kr", C.c_float), ("kb", C.c_float)]


class YccMergeDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("r", C.c_int), ("kr", C.c_float), ("kb", C.c_float)]


class ChromaUpDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("r", C.c_int), ("dtype", C.c_int), ("maxval", C.c_int), ("shift", C.c_int),
                ("siting", C.c_int)]


class YuvRgbDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("r", C.c_int), ("dtype", C.c_int), ("maxval", C.c_int), ("shift", C.c_int),
                ("siting", C.c_int), ("range", C.c_int), ("kr", C.c_float), ("kb", C.c_float)]


class RgbCbcrDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("r", C.c_int), ("siting", C.c_int), ("range", C.c_int), ("kr", C.c_float), ("kb", C.c_float)]


class PlaneFitDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("OH", C.c_int), ("OW", C.c_int), ("dtype", C.c_int), ("maxval", C.c_int), ("shift", C.c_int),
                ("siting", C.c_int)]


class YuvTensorDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("OH", C.c_int), ("OW", C.c_int), ("C", C.c_int), ("src_dtype", C.c_int), ("out_dtype", C.c_int), ("maxval", C.c_int),
                ("shift", C.c_int), ("siting", C.c_int), ("range", C.c_int), ("kr", C.c_float), ("kb", C.c_float), ("filter", C.c_int), ("means", C.c_float * 3),
                ("norms", C.c_float * 3), ("alpha", C.c_float)]


class RgbFitDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("OH", C.c_int), ("OW", C.c_int), ("C", C.c_int), ("source", C.c_int), ("dtype", C.c_int), ("maxval", C.c_int),
                ("shift", C.c_int), ("siting", C.c_int), ("range", C.c_int), ("kr", C.c_float), ("kb", C.c_float)]


class TensorYuvDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("in_dtype", C.c_int), ("out_dtype", C.c_int), ("maxval", C.c_int), ("shift", C.c_int),
                ("siting", C.c_int), ("range", C.c_int), ("kr", C.c_float), ("kb", C.c_float), ("scale", C.c_float * 3), ("offset", C.c_float * 3)]


class FrameMetricsDesc(C.Structure):
    _fields_ = [("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("dtype", C.c_int), ("maxval", C.c_int), ("shift", C.c_int)]


class FrameMetricsRow(C.Structure):
    _fields_ = [("sse", C.c_ulonglong), ("pixels", C.c_ulonglong), ("windows", C.c_ulonglong), ("ssim_sum", C.c_double)]


class DeviceInfo(C.Structure):
    _fields_ = [("name", C.c_char * 128), ("compute_units", C.c_int), ("lds_bytes_per_cu", C.c_int), ("hbm_bytes", C.c_size_t), ("device", C.c_int)]


_lib = None

_P = C.c_void_p
_FP = C.POINTER(C.c_float)


class GraphNode(C.Structure):
    _fields_ = [("plan", _P), ("n_inputs", C.c_int), ("inputs", C.c_int * 4), ("keep", C.c_int)]


class FusedNode(C.Structure):
    _fields_ = [("plan", _P), ("owned", C.c_int), ("n_inputs", C.c_int), ("inputs", C.c_int * 4)]


# name -> (restype, argtypes); must list every symbol include/snnhip.h declares (tests/test_abi.py checks that)
SIGNATURES = {
    "snnhip_ctx_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "snnhip_ctx_create_on_stream": (C.c_int, [C.c_int, _P, C.POINTER(_P)]),
    "snnhip_ctx_destroy": (C.c_int, [_P]),
    "snnhip_ctx_info": (C.c_int, [_P, C.POINTER(DeviceInfo)]),
    "snnhip_ctx_stream": (_P, [_P]),
    "snnhip_ctx_fork": (C.c_int, [_P]),
    "snnhip_ctx_main": (C.c_int, [_P]),
    "snnhip_ctx_join": (C.c_int, [_P]),
    "snnhip_ctx_group_begin": (C.c_int, [_P]),
    "snnhip_ctx_group_end": (C.c_int, [_P]),
    "snnhip_plan_groupable": (C.c_int, [_P]),
    "snnhip_sync": (C.c_int, [_P]),
    "snnhip_last_error": (C.c_char_p, []),
    "snnhip_version": (C.c_char_p, []),
    "snnhip_set_option": (C.c_int, [C.c_char_p, C.c_char_p]),
    "snnhip_guard_active": (C.c_int, []),
    "snnhip_guard_check": (C.c_int, [_P]),
    "snnhip_guard_selftest": (C.c_int, [_P, _P, C.c_long]),
    "snnhip_get_option": (C.c_char_p, [C.c_char_p]),
    "snnhip_tensor_alloc": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "snnhip_tensor_wrap": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "snnhip_tensor_free": (C.c_int, [_P]),
    "snnhip_tensor_dims": (C.c_int, [_P, C.POINTER(C.c_int * 4)]),
    "snnhip_tensor_data": (_P, [_P]),
    "snnhip_tensor_bytes": (C.c_size_t, [_P]),
    "snnhip_tensor_dtype": (C.c_int, [_P]),
    "snnhip_tensor_upload": (C.c_int, [_P, _FP]),
    "snnhip_tensor_download": (C.c_int, [_P, _FP]),
    "snnhip_tensor_upload_c4hw4": (C.c_int, [_P, _FP]),
    "snnhip_tensor_download_c4hw4": (C.c_int, [_P, _FP]),
    "snnhip_tensor_fill": (C.c_int, [_P, C.c_float]),
    "snnhip_conv2d_plan_create": (C.c_int, [_P, C.POINTER(ConvDesc), _FP, _FP, _FP, _FP, _FP, _FP, C.POINTER(_P)]),
    "snnhip_depthwise_plan_create": (C.c_int, [_P, C.POINTER(ConvDesc), _FP, _FP, _FP, _FP, _FP, _FP, C.POINTER(_P)]),
    "snnhip_dense_plan_create": (C.c_int, [_P, C.POINTER(DenseDesc), _FP, _FP, C.POINTER(_P)]),
    "snnhip_subpixel_plan_create": (C.c_int, [_P, C.POINTER(SubpixelDesc), C.POINTER(_P)]),
    "snnhip_add_plan_create": (C.c_int, [_P, C.POINTER(EltwiseDesc), C.POINTER(_P)]),
    "snnhip_activation_plan_create": (C.c_int, [_P, C.POINTER(EltwiseDesc), C.POINTER(_P)]),
    "snnhip_batchnorm_plan_create": (C.c_int, [_P, C.POINTER(EltwiseDesc), _FP, _FP, _FP, _FP, C.POINTER(_P)]),
    "snnhip_pool2d_plan_create": (C.c_int, [_P, C.POINTER(Pool2dDesc), C.POINTER(_P)]),
    "snnhip_pad_plan_create": (C.c_int, [_P, C.POINTER(PadDesc), C.POINTER(_P)]),
    "snnhip_upsample_plan_create": (C.c_int, [_P, C.POINTER(UpsampleDesc), C.POINTER(_P)]),
    "snnhip_instancenorm_plan_create": (C.c_int, [_P, C.POINTER(InstanceNormDesc), _FP, _FP, C.POINTER(_P)]),
    "snnhip_concat_plan_create": (C.c_int, [_P, C.POINTER(ConcatDesc), C.POINTER(_P)]),
    "snnhip_unary_plan_create": (C.c_int, [_P, C.POINTER(UnaryDesc), C.POINTER(_P)]),
    "snnhip_deconv2d_plan_create": (C.c_int, [_P, C.POINTER(ConvDesc), _FP, _FP, _FP, _FP, _FP, _FP, C.POINTER(_P)]),
    "snnhip_calculate_plan_create": (C.c_int, [_P, C.POINTER(CalculateDesc), C.POINTER(_P)]),
    "snnhip_resize_plan_create": (C.c_int, [_P, C.POINTER(ResizeDesc), C.POINTER(_P)]),
    "snnhip_image_u8_plan_create": (C.c_int, [_P, C.POINTER(ImageU8Desc), C.POINTER(_P)]),
    "snnhip_tensor_upload_raw": (C.c_int, [_P, _P, C.c_size_t]),
    "snnhip_tensor_download_raw": (C.c_int, [_P, _P, C.c_size_t]),
    "snnhip_u8_in_plan_create": (C.c_int, [_P, C.POINTER(U8InDesc), C.POINTER(_P)]),
    "snnhip_u8_out_plan_create": (C.c_int, [_P, C.POINTER(U8OutDesc), C.POINTER(_P)]),
    "snnhip_u16_in_plan_create": (C.c_int, [_P, C.POINTER(U16InDesc), C.POINTER(_P)]),
    "snnhip_u16_out_plan_create": (C.c_int, [_P, C.POINTER(U16OutDesc), C.POINTER(_P)]),
    "snnhip_rgb_luma_plan_create": (C.c_int, [_P, C.POINTER(RgbLumaDesc), C.POINTER(_P)]),
    "snnhip_ycc_merge_plan_create": (C.c_int, [_P, C.POINTER(YccMergeDesc), C.POINTER(_P)]),
    "snnhip_bicubic_taps": (C.c_int, [C.c_int, _FP, C.c_int]),
    "snnhip_chroma_up_plan_create": (C.c_int, [_P, C.POINTER(ChromaUpDesc), C.POINTER(_P)]),
    "snnhip_bicubic_taps_sited": (C.c_int, [C.c_int, C.c_int, _FP, C.POINTER(C.c_int), C.c_int]),
    "snnhip_yuv_rgb_plan_create": (C.c_int, [_P, C.POINTER(YuvRgbDesc), C.POINTER(_P)]),
    "snnhip_bicubic_taps_420": (C.c_int, [C.c_int, C.c_int, _FP, C.POINTER(C.c_int), C.c_int]),
    "snnhip_yuv_rgb_coefficients": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_float, _FP, C.c_int]),
    "snnhip_rgb_cbcr_plan_create": (C.c_int, [_P, C.POINTER(RgbCbcrDesc), C.POINTER(_P)]),
    "snnhip_bicubic_taps_rgb420": (C.c_int, [C.c_int, C.c_int, _FP, C.POINTER(C.c_int), C.c_int]),
    "snnhip_rgb_cbcr_coefficients": (C.c_int, [C.c_int, C.c_float, C.c_float, _FP, C.c_int]),
    "snnhip_yuv_rgb_planar_plan_create": (C.c_int, [_P, C.POINTER(YuvRgbDesc), C.POINTER(_P)]),
    "snnhip_rgb_cbcr_planar_plan_create": (C.c_int, [_P, C.POINTER(RgbCbcrDesc), C.POINTER(_P)]),
    "snnhip_plane_fit_plan_create": (C.c_int, [_P, C.POINTER(PlaneFitDesc), C.POINTER(_P)]),
    "snnhip_fit_taps": (C.c_int, [C.c_int, C.c_int, C.c_int, _FP, C.POINTER(C.c_int), C.c_int]),
    "snnhip_rgb_fit_plan_create": (C.c_int, [_P, C.POINTER(RgbFitDesc), C.POINTER(_P)]),
    "snnhip_rgb_fit_taps": (C.c_int, [C.c_int, C.c_int, C.c_int, _FP, C.POINTER(C.c_int), C.c_int]),
    "snnhip_yuv_tensor_plan_create": (C.c_int, [_P, C.POINTER(YuvTensorDesc), C.POINTER(_P)]),
    "snnhip_yuv_tensor_planar_plan_create": (C.c_int, [_P, C.POINTER(YuvTensorDesc), C.POINTER(_P)]),
    "snnhip_yuv_tensor_taps": (C.c_int, [C.c_int, C.c_int, C.c_int, _FP, C.POINTER(C.c_int), C.c_int]),
    "snnhip_tensor_yuv_plan_create": (C.c_int, [_P, C.POINTER(TensorYuvDesc), C.POINTER(_P)]),
    "snnhip_tensor_yuv_planar_plan_create": (C.c_int, [_P, C.POINTER(TensorYuvDesc), C.POINTER(_P)]),
    "snnhip_tensor_yuv_coefficients": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_float, _FP, C.c_int]),
    "snnhip_frame_metrics_plan_create": (C.c_int, [_P, C.POINTER(FrameMetricsDesc), C.POINTER(_P)]),
    "snnhip_frame_metrics_read": (C.c_int, [_P, C.POINTER(FrameMetricsRow), C.c_int]),
    "snnhip_frame_metrics_psnr": (C.c_double, [C.c_ulonglong, C.c_ulonglong, C.c_int]),
    "snnhip_tensor_argmax": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    "snnhip_chain_plan_create": (C.c_int, [_P, C.POINTER(_P), C.c_int, C.POINTER(_P)]),
    "snnhip_espcn_f16_pack_weights": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.POINTER(C.c_int)]),
    "snnhip_espcn_f16_wide_pack_weights": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.POINTER(C.c_int)]),
    "snnhip_graph_fuse": (C.c_int, [_P, C.POINTER(GraphNode), C.c_int, C.POINTER(FusedNode)]),
    "snnhip_plan_run": (C.c_int, [_P, _P, _P]),
    "snnhip_plan_run_n": (C.c_int, [_P, C.POINTER(_P), C.c_int, _P]),
    "snnhip_plan_run_io": (C.c_int, [_P, C.POINTER(_P), C.c_int, C.POINTER(_P), C.c_int]),
    "snnhip_plan_output_dims": (C.c_int, [_P, C.POINTER(C.c_int * 4)]),
    "snnhip_plan_describe": (C.c_int, [_P, C.c_char_p, C.c_size_t]),
    "snnhip_plan_cost": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "snnhip_plan_destroy": (C.c_int, [_P]),
    "snnhip_plan_num_steps": (C.c_int, [_P]),
    "snnhip_plan_step_describe": (C.c_int, [_P, C.c_int, C.c_char_p, C.c_size_t]),
    "snnhip_plan_step_cost": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "snnhip_plan_profile_enable": (C.c_int, [_P, C.c_int]),
    "snnhip_plan_profile_read": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "snnhip_graph_begin_capture": (C.c_int, [_P]),
    "snnhip_graph_end_capture": (C.c_int, [_P, C.POINTER(_P)]),
    "snnhip_graph_launch": (C.c_int, [_P]),
    "snnhip_graph_num_nodes": (C.c_int, [_P]),
    "snnhip_graph_destroy": (C.c_int, [_P]),
    "snnhip_timer_create": (C.c_int, [_P, C.POINTER(_P)]),
    "snnhip_timer_start": (C.c_int, [_P]),
    "snnhip_timer_stop": (C.c_int, [_P]),
    "snnhip_timer_elapsed_ms": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "snnhip_timer_destroy": (C.c_int, [_P]),
    "snnhip_trace_begin": (C.c_int, []),
    "snnhip_trace_end": (C.c_int, []),
    "snnhip_trace_report": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
}


def load_library():
    """Loads libsnnhip.so (built in-tree by __graft_entry__.build()).  torch is imported first so that the process has
    ONE HIP runtime: torch's bundled libamdhip64 has SONAME libamdhip64.so.7, which satisfies this library's
    DT_NEEDED; loading in the other order would map a second runtime."""
    global _lib
    if _lib is not None:
        return LIB_PATH
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` first" % LIB_PATH)
    import torch  # noqa: F401

    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return LIB_PATH


def lib():
    load_library()
    return _lib


def set_option(name, value):
    """snnhip_set_option: override a kernel-selection / fusion switch for this process; None removes the override (the environment
    variable of the same name is the fallback)."""
    check(lib().snnhip_set_option(name.encode(), None if value is None else str(value).encode()))


def get_option(name):
    v = lib().snnhip_get_option(name.encode())
    return None if v is None else v.decode()


def trace_begin():
    """snnhip_trace_begin: from now on every kernel the library launches is stamped with its own dispatch start / end and booked on its plan."""
    check(lib().snnhip_trace_begin())


def trace_end():
    """snnhip_trace_end + snnhip_trace_report: the launches since trace_begin grouped by kernel function (parsed JSON)."""
    import json

    check(lib().snnhip_trace_end())
    need = C.c_size_t(0)
    check(lib().snnhip_trace_report(None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value + 16)
    check(lib().snnhip_trace_report(buf, len(buf), C.byref(need)))
    return json.loads(buf.value.decode("utf-8", "replace"))


def check(rc):
    if rc != OK:
        raise SnnHipError(rc, lib().snnhip_last_error().decode("utf-8", "replace"))


def _fptr(a):
    if a is None:
        return None
    return a.ctypes.data_as(_FP)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


class Context:
    def __init__(self, device=0, stream=None):
        h = _P()
        if stream is None:
            check(lib().snnhip_ctx_create(device, C.byref(h)))
        else:
            check(lib().snnhip_ctx_create_on_stream(device, _P(stream), C.byref(h)))
        self.h = h
        self.device = device

    def info(self):
        di = DeviceInfo()
        check(lib().snnhip_ctx_info(self.h, C.byref(di)))
        return {"name": di.name.decode(), "compute_units": di.compute_units, "lds_bytes_per_cu": di.lds_bytes_per_cu, "hbm_bytes": di.hbm_bytes}

    def sync(self):
        check(lib().snnhip_sync(self.h))

    def stream(self):
        return lib().snnhip_ctx_stream(self.h)

    def fork(self):
        """plans run from now on go to the context's side stream (it first waits for the main stream's work so far)"""
        check(lib().snnhip_ctx_fork(self.h))

    def main(self):
        check(lib().snnhip_ctx_main(self.h))

    def join(self):
        """back on the main stream, which waits for the side stream's work"""
        check(lib().snnhip_ctx_join(self.h))

    def group_begin(self):
        """groupable plans (Plan.groupable()) run from now on are launched by group_end -- two that fit one grid as ONE kernel launch"""
        check(lib().snnhip_ctx_group_begin(self.h))

    def group_end(self):
        check(lib().snnhip_ctx_group_end(self.h))

    def close(self):
        if self.h:
            lib().snnhip_ctx_destroy(self.h)
            self.h = None


F32, F16, U8 = 0, 1, 2  # SNNHIP_F32 / SNNHIP_F16 / SNNHIP_U8 (8-bit frames: image_u8_plan / u8_in_plan input, u8_out_plan output)
U16 = 3  # SNNHIP_U16 (16-bit frames: u16_in_plan input, u16_out_plan output)


class Tensor:
    """NHWC tensor in HBM: fp32, or fp16 storage (dtype=F16; upload / numpy() still speak float32 and convert at the edge)."""

    def __init__(self, ctx, n, h, w, c, device_ptr=None, keepalive=None, dtype=F32):
        self.ctx = ctx
        self.shape = (n, h, w, c)
        self.dtype = dtype
        hh = _P()
        if device_ptr is None:
            check(lib().snnhip_tensor_alloc(ctx.h, n, h, w, c, dtype, C.byref(hh)))
        else:
            check(lib().snnhip_tensor_wrap(ctx.h, _P(device_ptr), n, h, w, c, dtype, C.byref(hh)))
        self.h = hh
        self._keepalive = keepalive

    @staticmethod
    def from_numpy(ctx, a, dtype=F32):
        """dtype=U8 / U16 (or a uint16 array): the array's bytes as an 8-bit / 16-bit frame tensor (uploaded raw)."""
        if dtype == U16 or (dtype == F32 and getattr(a, "dtype", None) == np.uint16):
            a = np.ascontiguousarray(a, dtype=np.uint16)
            assert a.ndim == 4, "expected NHWC"
            t = Tensor(ctx, *a.shape, dtype=U16)
            t.upload_u16(a)
            return t
        if dtype == U8:
            a = np.ascontiguousarray(a, dtype=np.uint8)
            assert a.ndim == 4, "expected NHWC"
            t = Tensor(ctx, *a.shape, dtype=U8)
            t.upload_u8(a)
            return t
        a = np.ascontiguousarray(a, dtype=np.float32)
        assert a.ndim == 4, "expected NHWC"
        t = Tensor(ctx, *a.shape, dtype=dtype)
        t.upload(a)
        return t

    @staticmethod
    def from_torch(ctx, tt):
        """Borrows the storage of a contiguous NHWC float32 torch tensor living on the context's device."""
        assert tt.is_contiguous() and tt.dim() == 4 and str(tt.dtype) == "torch.float32"
        n, h, w, c = tt.shape
        return Tensor(ctx, n, h, w, c, device_ptr=tt.data_ptr(), keepalive=tt)

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        assert a.size == int(np.prod(self.shape)), (a.shape, self.shape)
        check(lib().snnhip_tensor_upload(self.h, _fptr(a)))

    def numpy(self):
        out = np.empty(self.shape, dtype=np.float32)
        check(lib().snnhip_tensor_download(self.h, _fptr(out)))
        return out

    def upload_u8(self, a):
        """Raw byte upload of an 8-bit image tensor (dtype=U8)."""
        a = np.ascontiguousarray(a, dtype=np.uint8)
        assert self.dtype == U8 and a.size == int(np.prod(self.shape)), (a.shape, self.shape)
        check(lib().snnhip_tensor_upload_raw(self.h, a.ctypes.data_as(_P), a.size))

    def numpy_u8(self):
        """Raw byte download of an 8-bit tensor (dtype=U8) as uint8 NHWC (numpy() speaks float32 and refuses 8-bit tensors)."""
        assert self.dtype == U8, self.dtype
        out = np.empty(self.shape, dtype=np.uint8)
        check(lib().snnhip_tensor_download_raw(self.h, out.ctypes.data_as(_P), out.size))
        return out

    def upload_u16(self, a):
        """Raw upload of a 16-bit frame tensor (dtype=U16)."""
        a = np.ascontiguousarray(a, dtype=np.uint16)
        assert self.dtype == U16 and a.size == int(np.prod(self.shape)), (a.shape, self.shape)
        check(lib().snnhip_tensor_upload_raw(self.h, a.ctypes.data_as(_P), a.nbytes))

    def numpy_u16(self):
        """Raw download of a 16-bit frame tensor (dtype=U16) as uint16 NHWC (numpy() speaks float32 and refuses frame tensors)."""
        assert self.dtype == U16, self.dtype
        out = np.empty(self.shape, dtype=np.uint16)
        check(lib().snnhip_tensor_download_raw(self.h, out.ctypes.data_as(_P), out.nbytes))
        return out

    def argmax(self, n=0):
        """Index of the largest element of image n (first on ties) -- the reference reports this + 1 as classifierOutput (core.cpp:228-234)."""
        out = C.c_int(-1)
        check(lib().snnhip_tensor_argmax(self.h, n, C.byref(out)))
        return out.value

    def upload_c4hw4(self, a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        check(lib().snnhip_tensor_upload_c4hw4(self.h, _fptr(a)))

    def numpy_c4hw4(self):
        n, h, w, c = self.shape
        out = np.empty((n, (c + 3) // 4, h, w, 4), dtype=np.float32)
        check(lib().snnhip_tensor_download_c4hw4(self.h, _fptr(out)))
        return out

    def fill(self, v):
        check(lib().snnhip_tensor_fill(self.h, float(v)))

    def data_ptr(self):
        return lib().snnhip_tensor_data(self.h)

    def free(self):
        if self.h:
            lib().snnhip_tensor_free(self.h)
            self.h = None


class Plan:
    def __init__(self, ctx, handle, keep=()):
        self.ctx = ctx
        self.h = handle
        self._keep = keep

    def out_shape(self):
        d = (C.c_int * 4)()
        check(lib().snnhip_plan_output_dims(self.h, C.byref(d)))
        return tuple(d)

    def describe(self):
        buf = C.create_string_buffer(2048)
        check(lib().snnhip_plan_describe(self.h, buf, 2048))
        return buf.value.decode()

    def cost(self):
        f, b = C.c_double(), C.c_double()
        check(lib().snnhip_plan_cost(self.h, C.byref(f), C.byref(b)))
        return f.value, b.value

    def run(self, x, y):
        if isinstance(x, (list, tuple)):
            arr = (_P * len(x))(*[t.h for t in x])
            check(lib().snnhip_plan_run_n(self.h, arr, len(x), y.h))
        else:
            check(lib().snnhip_plan_run(self.h, x.h, y.h))

    def run_io(self, xs, ys):
        """snnhip_plan_run_io: a plan with more than one output (tensor_yuv_plan); xs and ys are lists of tensors"""
        a = (_P * max(len(xs), 1))(*[t.h for t in xs])
        b = (_P * max(len(ys), 1))(*[t.h for t in ys])
        check(lib().snnhip_plan_run_io(self.h, a, len(xs), b, len(ys)))

    def __call__(self, x, y=None):
        if y is None:
            first = x[0] if isinstance(x, (list, tuple)) else x
            y = Tensor(self.ctx, *self.out_shape(), dtype=first.dtype)
        self.run(x, y)
        return y

    def groupable(self):
        return bool(lib().snnhip_plan_groupable(self.h))

    def num_steps(self):
        return lib().snnhip_plan_num_steps(self.h)

    def step_describe(self, i):
        buf = C.create_string_buffer(1024)
        check(lib().snnhip_plan_step_describe(self.h, i, buf, 1024))
        return buf.value.decode()

    def step_cost(self, i):
        f, b = C.c_double(), C.c_double()
        check(lib().snnhip_plan_step_cost(self.h, i, C.byref(f), C.byref(b)))
        return f.value, b.value

    def profile(self, enable=True):
        check(lib().snnhip_plan_profile_enable(self.h, int(enable)))

    def profile_read(self, i):
        """(total_ms, launches) of step i since the last read."""
        ms, n = C.c_double(), C.c_int()
        check(lib().snnhip_plan_profile_read(self.h, i, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def destroy(self):
        if self.h:
            lib().snnhip_plan_destroy(self.h)
            self.h = None


def _conv_desc(N, H, W, IC, OC, k, stride, pads, pad_mode, act, leaky, use_bias, use_bn, OH=0, OW=0):
    d = ConvDesc()
    d.N, d.H, d.W, d.IC, d.OC = N, H, W, IC, OC
    kh, kw = (k, k) if isinstance(k, int) else k
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    d.kh, d.kw, d.sh, d.sw = kh, kw, sh, sw
    d.padT, d.padB, d.padL, d.padR = pads
    d.padMode = PAD_MODE[pad_mode] if isinstance(pad_mode, str) else pad_mode
    d.act = ACT[act] if isinstance(act, str) else act
    d.leaky = leaky
    d.useBias, d.useBN, d.dtype, d.OH, d.OW = int(use_bias), int(use_bn), 0, OH, OW
    return d


def same_padding(k):
    """Conv2DLayer::getPaddingOffset for padding "same" (reference conv2d.cpp:57-66): returns (T, B, L, R)."""
    if k > 1:
        p = max(k // 2, 1)
        t = [p, p, p, p]
        if k % 2 == 0:
            t[0] -= 1
            t[2] -= 1
        return tuple(t)
    return (0, 0, 0, 0)


def conv2d_plan(ctx, N, H, W, w_oihw, bias=None, stride=1, pads=None, pad_mode="constant", act="", leaky=0.0, bn=None, depthwise=False, dtype=F32):
    """w_oihw: [OC][IC][kh][kw] (depthwise: [C][kh][kw]). bn: dict beta/gamma/mean/var or None. pads: (T,B,L,R) or None=same."""
    w = _f32(w_oihw)
    if depthwise:
        OC, kh, kw = w.shape
        IC = OC
    else:
        OC, IC, kh, kw = w.shape
    if pads is None:
        pads = same_padding(kh)
    b = _f32(bias)
    bnp = [None] * 4
    if bn is not None:
        bnp = [_f32(bn[k]) for k in ("beta", "gamma", "mean", "var")]
    d = _conv_desc(N, H, W, IC, OC, (kh, kw), stride, pads, pad_mode, act, leaky, b is not None, bn is not None)
    d.dtype = dtype
    h = _P()
    fn = lib().snnhip_depthwise_plan_create if depthwise else lib().snnhip_conv2d_plan_create
    check(fn(ctx.h, C.byref(d), _fptr(w), _fptr(b), _fptr(bnp[0]), _fptr(bnp[1]), _fptr(bnp[2]), _fptr(bnp[3]), C.byref(h)))
    return Plan(ctx, h)


def dense_plan(ctx, batch, w_flat, out_units, bias=None, act="", leaky=0.0):
    w = _f32(w_flat).reshape(-1)
    in_units = w.size // out_units
    d = DenseDesc(batch, in_units, out_units, DENSE_ACT[act] if isinstance(act, str) else act, leaky, int(bias is not None))
    b = _f32(bias)
    h = _P()
    check(lib().snnhip_dense_plan_create(ctx.h, C.byref(d), _fptr(w), _fptr(b), C.byref(h)))
    return Plan(ctx, h)


def subpixel_plan(ctx, N, H, W, Cc, factor=2, mode=0):
    d = SubpixelDesc(N, H, W, Cc, factor, mode)
    h = _P()
    check(lib().snnhip_subpixel_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def _act_id(act):
    ids = {"": 0, "linear": 0, "none": 0, "relu": 1, "relu6": 2, "tanh": 3, "sigmoid": 4, "leakyRelu": 5, "SiLU": 6}
    return ids[act]


def add_plan(ctx, N, H, W, Cc, act="", leaky=0.0):
    """y = act(a + b); run with plan([a, b]).  (AddLayerVulkan, vk_add.comp)"""
    d = EltwiseDesc(N, H, W, Cc, _act_id(act), leaky)
    h = _P()
    check(lib().snnhip_add_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def activation_plan(ctx, N, H, W, Cc, act, leaky=0.0):
    d = EltwiseDesc(N, H, W, Cc, _act_id(act), leaky)
    h = _P()
    check(lib().snnhip_activation_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def batchnorm_plan(ctx, N, H, W, Cc, bn, act="", leaky=0.0):
    d = EltwiseDesc(N, H, W, Cc, _act_id(act), leaky)
    arrs = [_f32(bn[k]) for k in ("beta", "gamma", "mean", "var")]
    h = _P()
    check(lib().snnhip_batchnorm_plan_create(ctx.h, C.byref(d), *[_fptr(a) for a in arrs], C.byref(h)))
    return Plan(ctx, h)


def pool2d_plan(ctx, N, H, W, Cc, k, stride, kind="max", same=True, pad_t=0, pad_l=0, OH=0, OW=0):
    """kind 'max' | 'avg'.  `same` only selects the reference's output-size rule; the window is always clipped to the image."""
    d = Pool2dDesc(N, H, W, Cc, k, k, stride, stride, pad_t, pad_l, OH, OW, int(bool(same)), 0 if kind == "max" else 1)
    h = _P()
    check(lib().snnhip_pool2d_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def global_avgpool_plan(ctx, N, H, W, Cc):
    """AdaptiveAvgPool2d with target 1: the mean over the whole image (adaptiveavgpool2dGL.cpp)."""
    d = Pool2dDesc(N, H, W, Cc, H, W, H, W, 0, 0, 1, 1, 0, 1)
    h = _P()
    check(lib().snnhip_pool2d_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def pad_plan(ctx, N, H, W, Cc, pads, mode="constant"):
    """pads = (T, B, L, R); mode constant | replicate | reflect."""
    d = PadDesc(N, H, W, Cc, pads[0], pads[1], pads[2], pads[3], {"constant": 0, "replicate": 1, "reflect": 2}[mode])
    h = _P()
    check(lib().snnhip_pad_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def upsample_plan(ctx, N, H, W, Cc, scale=2.0, mode="nearest"):
    d = UpsampleDesc(N, H, W, Cc, scale, {"nearest": 0, "bilinear": 1}[mode])
    h = _P()
    check(lib().snnhip_upsample_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def instancenorm_plan(ctx, N, H, W, Cc, beta, gamma, act="", leaky=0.0, eps=1e-5):
    d = InstanceNormDesc(N, H, W, Cc, _act_id(act), leaky, eps)
    b, g = _f32(beta), _f32(gamma)
    h = _P()
    check(lib().snnhip_instancenorm_plan_create(ctx.h, C.byref(d), _fptr(b), _fptr(g), C.byref(h)))
    return Plan(ctx, h)


def concat_plan(ctx, N, H, W, C0, C1, OC=None):
    d = ConcatDesc(N, H, W, C0, C1, C0 + C1 if OC is None else OC)
    h = _P()
    check(lib().snnhip_concat_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


UNARY_OPS = {"copy": 0, "fixed": 1, "neg": 2, "rcp": 3, "square": 4, "exp": 5, "abs": 6}


def unary_plan(ctx, N, H, W, Cc, op="copy", value=1.0):
    d = UnaryDesc(N, H, W, Cc, UNARY_OPS[op] if isinstance(op, str) else int(op), value)
    h = _P()
    check(lib().snnhip_unary_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def calculate_plan(ctx, N, H, W, Cc, OC):
    d = CalculateDesc(N, H, W, Cc, OC)
    h = _P()
    check(lib().snnhip_calculate_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def resize_plan(ctx, N, H, W, Cc, OH, OW, means=(0, 0, 0, 0), norms=(1, 1, 1, 1), linear=True):
    d = ResizeDesc(N, H, W, Cc, OH, OW, (C.c_float * 4)(*means), (C.c_float * 4)(*norms), 1 if linear else 0)
    h = _P()
    check(lib().snnhip_resize_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def image_u8_plan(ctx, N, H, W, src_channels, means=(0, 0, 0, 0), norms=(1, 1, 1, 1)):
    d = ImageU8Desc(N, H, W, src_channels, (C.c_float * 4)(*means), (C.c_float * 4)(*norms))
    h = _P()
    check(lib().snnhip_image_u8_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def u8_in_plan(ctx, N, H, W, Cc, means=(0, 0, 0, 0), norms=(1, 1, 1, 1), dtype=F32):
    """U8 [N][H][W][Cc] -> dtype [N][H][W][Cc]: y = (float(u) - means[c]) * norms[c]."""
    d = U8InDesc(N, H, W, Cc, dtype, (C.c_float * 4)(*means), (C.c_float * 4)(*norms))
    h = _P()
    check(lib().snnhip_u8_in_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def u16_in_plan(ctx, N, H, W, Cc, means=(0, 0, 0, 0), norms=(1, 1, 1, 1), shift=0, dtype=F32):
    """U16 [N][H][W][Cc] -> dtype [N][H][W][Cc]: y = (float(u >> shift) - means[c]) * norms[c]."""
    d = U16InDesc(N, H, W, Cc, dtype, (C.c_float * 4)(*means), (C.c_float * 4)(*norms), shift)
    h = _P()
    check(lib().snnhip_u16_in_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def u16_out_plan(ctx, N, H, W, Cc, scale=(1, 1, 1, 1), offset=(0, 0, 0, 0), maxval=65535, shift=0, dtype=F32):
    """dtype [N][H][W][Cc] -> U16: q = unsigned(clamp(rint(fmaf(x, scale[c], offset[c])), 0, maxval)) << shift, NaN -> 0."""
    d = U16OutDesc(N, H, W, Cc, dtype, (C.c_float * 4)(*scale), (C.c_float * 4)(*offset), maxval, shift)
    h = _P()
    check(lib().snnhip_u16_out_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def u8_out_plan(ctx, N, H, W, Cc, scale=(1, 1, 1, 1), offset=(0, 0, 0, 0), dtype=F32):
    """dtype [N][H][W][Cc] -> U8: q = clamp(rint(fmaf(x, scale[c], offset[c])), 0, 255), NaN -> 0."""
    d = U8OutDesc(N, H, W, Cc, dtype, (C.c_float * 4)(*scale), (C.c_float * 4)(*offset))
    h = _P()
    check(lib().snnhip_u8_out_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


BT601 = (0.299, 0.114)  # (kr, kb): what cv2.COLOR_BGR2YCrCb uses; BT.709 is (0.2126, 0.0722)


def rgb_luma_plan(ctx, N, H, W, Cc, kr=BT601[0], kb=BT601[1]):
    """U8 [N][H][W][Cc] (Cc = 3 RGB, 4 RGBA) -> U8 [N][H][W][1]: q = clamp(rint(kr*R + kg*G + kb*B), 0, 255), kg = 1 - kr - kb."""
    d = RgbLumaDesc(N, H, W, Cc, kr, kb)
    h = _P()
    check(lib().snnhip_rgb_luma_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def ycc_merge_plan(ctx, N, H, W, Cc, r, kr=BT601[0], kb=BT601[1]):
    """plan.run([Yhi U8 [N][r*H][r*W][1], frame U8 [N][H][W][Cc]], out U8 [N][r*H][r*W][Cc]): the frame's chroma, bicubically upsampled, around Yhi
    (include/snnhip.h states the arithmetic).  H, W are the LOW-resolution frame's."""
    d = YccMergeDesc(N, H, W, Cc, r, kr, kb)
    h = _P()
    check(lib().snnhip_ycc_merge_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def bicubic_taps(r):
    """snnhip_bicubic_taps (host side only, no GPU): the [r][4] float32 Catmull-Rom weight table of an r-fold upscale, row p = phase X mod r."""
    out = np.zeros((r, 4), np.float32)
    check(lib().snnhip_bicubic_taps(r, _fptr(out), out.size))
    return out


SITING = {"centre": 0, "left": 1}  # SNNHIP_SITING_*


def chroma_up_plan(ctx, N, H, W, Cc, r, dtype=U8, maxval=None, shift=0, siting="left"):
    """dtype (U8 / U16) [N][H][W][Cc] -> [N][r*H][r*W][Cc]: a chroma plane (Cc = 2 interleaved CbCr, 1 one planar plane; H, W its own extent)
    upsampled with the sited Catmull-Rom filter of include/snnhip.h; maxval defaults to 255 for U8 (a 16-bit plane must say: 1023 or 4095)."""
    if maxval is None:
        maxval = 255
    d = ChromaUpDesc(N, H, W, Cc, r, dtype, maxval, shift, SITING.get(siting, siting))
    h = _P()
    check(lib().snnhip_chroma_up_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def bicubic_taps_sited(r, siting="left"):
    """snnhip_bicubic_taps_sited (host side only, no GPU): (weights float32 [r][4], base int32 [r]); phase p reads x + base[p] - 1 .. x + base[p] + 2."""
    w = np.zeros((max(r, 0), 4), np.float32)
    base = (C.c_int * max(r, 1))()
    check(lib().snnhip_bicubic_taps_sited(r, SITING.get(siting, siting), _fptr(w), base, w.size))
    return w, np.array(base[:max(r, 0)], np.int32)


RANGE = {"limited": 0, "full": 1}  # SNNHIP_RANGE_*


def yuv_rgb_plan(ctx, N, H, W, Cc, r, dtype=U8, maxval=None, shift=0, siting="left", range="limited", kr=BT601[0], kb=BT601[1]):
    """plan.run([Yhi [N][2r*H][2r*W][1], CbCr [N][H][W][2]], out [N][2r*H][2r*W][Cc]), all of dtype U8 / U16: a 4:2:0 frame to RGB (Cc = 3) or RGBA
    (Cc = 4) in one launch (include/snnhip.h states the arithmetic).  H, W are the CHROMA plane's; maxval defaults to 255 (a 16-bit frame must say)."""
    if maxval is None:
        maxval = 255
    d = YuvRgbDesc(N, H, W, Cc, r, dtype, maxval, shift, SITING.get(siting, siting), RANGE.get(range, range), kr, kb)
    h = _P()
    check(lib().snnhip_yuv_rgb_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def bicubic_taps_420(r, siting="left", capacity=None):
    """snnhip_bicubic_taps_420 (host side only, no GPU): (weights float32 [2r][4], base int32 [2r]) of a chroma plane resampled to the output luma
    grid; phase p = X mod 2r reads x + base[p] - 1 .. x + base[p] + 2."""
    n = 2 * max(r, 0)
    w = np.zeros((n, 4), np.float32)
    base = (C.c_int * max(n, 1))()
    check(lib().snnhip_bicubic_taps_420(r, SITING.get(siting, siting), _fptr(w), base, w.size if capacity is None else capacity))
    return w, np.array(base[:n], np.int32)


def yuv_rgb_coefficients(maxval=255, range="limited", kr=BT601[0], kb=BT601[1]):
    """snnhip_yuv_rgb_coefficients (host side only, no GPU): float32 (Yoff, Coff, cy, crv, cbu, cgv, cgu) of the Y'CbCr -> RGB matrix."""
    out = np.zeros(7, np.float32)
    check(lib().snnhip_yuv_rgb_coefficients(maxval, RANGE.get(range, range), kr, kb, _fptr(out), out.size))
    return out


def rgb_cbcr_plan(ctx, N, H, W, Cc, r, siting="left", range="limited", kr=BT601[0], kb=BT601[1]):
    """plan.run([frame U8 [N][H][W][Cc]], out U8 [N][r*H/2][r*W/2][2]): the CbCr plane of the r-fold upscaled 4:2:0 frame from the low-resolution RGB
    (Cc = 3) or RGBA (Cc = 4) frame, r = 2..4, in one launch (include/snnhip.h states the arithmetic)."""
    d = RgbCbcrDesc(N, H, W, Cc, r, SITING.get(siting, siting), RANGE.get(range, range), kr, kb)
    h = _P()
    check(lib().snnhip_rgb_cbcr_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def rgb420_phases(r):
    """rows of snnhip_bicubic_taps_rgb420's table: the output chroma pattern repeats every r / gcd(r, 2) samples"""
    return r if r % 2 else r // 2


def bicubic_taps_rgb420(r, siting="left", capacity=None):
    """snnhip_bicubic_taps_rgb420 (host side only, no GPU): (weights float32 [P][4], base int32 [P]), P = 1, 3, 2 for r = 2, 3, 4; output P x' + p
    of the upscaled frame's chroma grid reads low-resolution pixels S x' + base[p] - 1 .. S x' + base[p] + 2, S = 1, 2, 1."""
    n = rgb420_phases(r) if 2 <= r <= 4 else 0
    w = np.zeros((n, 4), np.float32)
    base = (C.c_int * max(n, 1))()
    check(lib().snnhip_bicubic_taps_rgb420(r, SITING.get(siting, siting), _fptr(w), base, w.size if capacity is None else capacity))
    return w, np.array(base[:n], np.int32)


def rgb_cbcr_coefficients(range="limited", kr=BT601[0], kb=BT601[1]):
    """snnhip_rgb_cbcr_coefficients (host side only, no GPU): float32 (Coff, cbs, crs) of the full-range differences -> CbCr codes map."""
    out = np.zeros(3, np.float32)
    check(lib().snnhip_rgb_cbcr_coefficients(RANGE.get(range, range), kr, kb, _fptr(out), out.size))
    return out


def yuv_rgb_planar_plan(ctx, N, H, W, Cc, r, dtype=U8, maxval=None, shift=0, siting="left", range="limited", kr=BT601[0], kb=BT601[1]):
    """plan.run([Yhi [N][2r*H][2r*W][1], chroma [2N][H][W][1]], out [N][2r*H][2r*W][Cc]): yuv_rgb_plan for planar chroma (I420 / I010): plane 2n is
    the Cb plane of image n, 2n + 1 its Cr plane.  One launch, the arithmetic of yuv_rgb_plan."""
    if maxval is None:
        maxval = 255
    d = YuvRgbDesc(N, H, W, Cc, r, dtype, maxval, shift, SITING.get(siting, siting), RANGE.get(range, range), kr, kb)
    h = _P()
    check(lib().snnhip_yuv_rgb_planar_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def rgb_cbcr_planar_plan(ctx, N, H, W, Cc, r, siting="left", range="limited", kr=BT601[0], kb=BT601[1]):
    """plan.run([frame U8 [N][H][W][Cc]], out U8 [2N][r*H/2][r*W/2][1]): rgb_cbcr_plan with a planar output (I420): plane 2n is the Cb plane of image
    n, 2n + 1 its Cr plane.  One launch, the arithmetic of rgb_cbcr_plan, r = 2..4."""
    d = RgbCbcrDesc(N, H, W, Cc, r, SITING.get(siting, siting), RANGE.get(range, range), kr, kb)
    h = _P()
    check(lib().snnhip_rgb_cbcr_planar_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def plane_fit_plan(ctx, N, H, W, Cc, OH, OW, dtype=U8, maxval=None, shift=0, siting="left"):
    """plan.run([plane [N][H][W][Cc]], out [N][OH][OW][Cc]): a U8 / U16 plane (Cc = 1: luma or one planar chroma plane, 2: interleaved CbCr) resampled
    to OH x OW, 1/2 <= OH / H, OW / W <= 4, with the stretched Keys cubic of include/snnhip.h; siting "left" or "centre" (the horizontal axis)."""
    if maxval is None:
        maxval = 255 if dtype == U8 else 1023
    d = PlaneFitDesc(N, H, W, Cc, OH, OW, dtype, maxval, shift, SITING.get(siting, siting))
    h = _P()
    check(lib().snnhip_plane_fit_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def fit_taps(n_in, n_out, siting="centre", capacity=None):
    """snnhip_fit_taps (host side only, no GPU): (weights float32 [n_out][8], base int32 [n_out]) of one axis; output X reads
    in[clamp(base[X] - 3 + k)] with weights[X][k]."""
    n = max(int(n_out), 0)
    w = np.zeros((n, 8), np.float32)
    base = (C.c_int * max(n, 1))()
    check(lib().snnhip_fit_taps(n_in, n_out, SITING.get(siting, siting), _fptr(w), base, w.size if capacity is None else capacity))
    return w, np.array(base[:n], np.int32)


YUV_TENSOR_FILTER = {"nearest": 0, "linear": 1}  # SNNHIP_YUV_TENSOR_*


def yuv_tensor_plan(ctx, N, H, W, OH, OW, Cc, src_dtype=U8, out_dtype=F32, maxval=None, shift=0, siting="left", range="limited", kr=BT601[0], kb=BT601[1], filter="linear",
                    means=(0, 0, 0), norms=(1, 1, 1), alpha=1.0, planar=False):
    """plan.run([Y [N][H][W][1], chroma], out [N][OH][OW][Cc]): a 4:2:0 video frame (U8 / U16 planes, H and W even) straight to the normalised fp32 /
    fp16 input tensor of an RGB (Cc = 3) or RGBA (Cc = 4) model at the model's input size, in one launch (include/snnhip.h states the arithmetic).
    The chroma is interleaved CbCr [N][H/2][W/2][2], or with planar=True [2N][H/2][W/2][1] (plane 2n = Cb, 2n + 1 = Cr).  H, W are the LUMA
    plane's; maxval defaults to 255 (a 16-bit frame must say)."""
    if maxval is None:
        maxval = 255
    d = YuvTensorDesc(N, H, W, OH, OW, Cc, src_dtype, out_dtype, maxval, shift, SITING.get(siting, siting), RANGE.get(range, range), kr, kb, YUV_TENSOR_FILTER.get(filter, filter),
                      (C.c_float * 3)(*means[:3]), (C.c_float * 3)(*norms[:3]), alpha)
    h = _P()
    check((lib().snnhip_yuv_tensor_planar_plan_create if planar else lib().snnhip_yuv_tensor_plan_create)(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def yuv_tensor_taps(n_in, n_out, filter="linear", capacity=None):
    """snnhip_yuv_tensor_taps (host side only, no GPU): (a float32 [n_out], index int32 [n_out][2]) of one axis: output o blends source samples
    index[o][0] and index[o][1] (already clamped) with weights 1 - a[o] and a[o]; nearest: the source index twice and a = 0."""
    n = max(int(n_out), 0)
    a = np.zeros(max(n, 1), np.float32)
    idx = (C.c_int * (2 * max(n, 1)))()
    check(lib().snnhip_yuv_tensor_taps(n_in, n_out, YUV_TENSOR_FILTER.get(filter, filter), _fptr(a), idx, n if capacity is None else capacity))
    return a[:n], np.array(idx[:2 * n], np.int32).reshape(n, 2)


def tensor_yuv_plan(ctx, N, H, W, Cc, in_dtype=F32, out_dtype=U8, maxval=None, shift=0, siting="left", range="limited", kr=BT601[0], kb=BT601[1], scale=(1, 1, 1),
                    offset=(0, 0, 0), planar=False):
    """plan.run_io([T [N][H][W][Cc]], [Y [N][H][W][1], chroma]): the fp32 / fp16 output tensor of an RGB (Cc = 3) or RGBA (Cc = 4, channel 3 ignored) model
    straight to the planes of a 4:2:0 video frame of the same extent (U8 / U16, H and W even), in one launch (include/snnhip.h states the arithmetic).
    The chroma is interleaved CbCr [N][H/2][W/2][2], or with planar=True [2N][H/2][W/2][1] (plane 2n = Cb, 2n + 1 = Cr); p = clamp(x * scale + offset,
    0, maxval) is full-range RGB at the output depth.  maxval defaults to 255 (a 16-bit frame must say)."""
    if maxval is None:
        maxval = 255
    d = TensorYuvDesc(N, H, W, Cc, in_dtype, out_dtype, maxval, shift, SITING.get(siting, siting), RANGE.get(range, range), kr, kb, (C.c_float * 3)(*scale[:3]),
                      (C.c_float * 3)(*offset[:3]))
    h = _P()
    check((lib().snnhip_tensor_yuv_planar_plan_create if planar else lib().snnhip_tensor_yuv_plan_create)(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def tensor_yuv_coefficients(maxval=255, range="limited", kr=BT601[0], kb=BT601[1], capacity=None):
    """snnhip_tensor_yuv_coefficients (host side only, no GPU): float32 (Yoff, ys, Coff, cbs, crs) of the full-range RGB -> Y'CbCr codes map."""
    out = np.zeros(5, np.float32)
    check(lib().snnhip_tensor_yuv_coefficients(maxval, RANGE.get(range, range), kr, kb, _fptr(out), out.size if capacity is None else capacity))
    return out


RGB_FIT_SOURCE = {"cbcr": 0, "planar": 1, "rgb": 2}  # SNNHIP_RGB_FIT_*


def rgb_fit_plan(ctx, N, H, W, OH, OW, Cc, source="cbcr", dtype=U8, maxval=None, shift=0, siting="left", range="limited", kr=BT601[0], kb=BT601[1]):
    """plan.run([Yfit [N][OH][OW][1], the chroma source], out [N][OH][OW][Cc]): packed RGB (Cc = 3) or RGBA (Cc = 4) at any output size from the luma
    frame already at that size and the ORIGINAL chroma source, enlarged 1- to 8-fold, in one launch (include/snnhip.h states the arithmetic).
    source "cbcr": CbCr [N][H][W][2]; "planar": [2N][H][W][1], plane 2n = Cb, 2n + 1 = Cr; "rgb": the U8 colour frame [N][H][W][Cc].  H, W are the
    source's extent; maxval defaults to 255 (a 16-bit frame must say)."""
    if maxval is None:
        maxval = 255
    d = RgbFitDesc(N, H, W, OH, OW, Cc, RGB_FIT_SOURCE.get(source, source), dtype, maxval, shift, SITING.get(siting, siting), RANGE.get(range, range), kr, kb)
    h = _P()
    check(lib().snnhip_rgb_fit_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def rgb_fit_taps(n_in, n_out, siting="centre", capacity=None):
    """snnhip_rgb_fit_taps (host side only, no GPU): (weights float32 [n_out][4], base int32 [n_out]) of one enlarging axis to the luma grid; output
    X reads in[clamp(base[X] - 1 + k)] with weights[X][k]; siting "left" is the horizontal axis of a left-sited 4:2:0 plane."""
    n = max(int(n_out), 0)
    w = np.zeros((n, 4), np.float32)
    base = (C.c_int * max(n, 1))()
    check(lib().snnhip_rgb_fit_taps(n_in, n_out, SITING.get(siting, siting), _fptr(w), base, w.size if capacity is None else capacity))
    return w, np.array(base[:n], np.int32)


FRAME_METRICS_TILE = (32, 128)  # (rows, columns) of pixels one block of frame_metrics_tile_kernel owns (csrc/frame_metrics.h); the plan's description carries it


def frame_metrics_plan(ctx, N, H, W, Cc, dtype=U8, maxval=None, shift=0):
    """snnhip_frame_metrics_plan_create: PSNR and SSIM of a test frame against a reference frame, per image and channel.  Run it with
    plan([test, reference], out), out an F32 tensor [N][1][C][2] = {psnr_db, ssim}; frame_metrics_read(plan) gives the exact rows."""
    d = FrameMetricsDesc()
    d.N, d.H, d.W, d.C, d.dtype, d.shift = N, H, W, Cc, dtype, shift
    d.maxval = (255 if dtype == U8 else 65535) if maxval is None else maxval
    h = _P()
    check(lib().snnhip_frame_metrics_plan_create(ctx.h, C.byref(d), C.byref(h)))
    return Plan(ctx, h)


def frame_metrics_read(plan, max_rows=None):
    """snnhip_frame_metrics_read: waits for the context's stream; one dict {sse, pixels, windows, ssim_sum, ssim} per (image, channel), image-major."""
    n, _, c, _ = plan.out_shape()
    rows = (FrameMetricsRow * (n * c if max_rows is None else max(max_rows, 1)))()
    got = lib().snnhip_frame_metrics_read(plan.h, rows, n * c if max_rows is None else max_rows)
    if got < 0:
        check(got)
    return [{"sse": r.sse, "pixels": r.pixels, "windows": r.windows, "ssim_sum": r.ssim_sum, "ssim": r.ssim_sum / r.windows} for r in rows[:got]]


def frame_metrics_psnr(sse, pixels, maxval):
    """snnhip_frame_metrics_psnr: 10 log10(maxval^2 pixels / sse) in double, inf for sse == 0 (host side, no device)."""
    return lib().snnhip_frame_metrics_psnr(int(sse), int(pixels), int(maxval))


def deconv2d_plan(ctx, N, H, W, w_oihw, bias=None, stride=2, same=True, act="", leaky=0.0, bn=None):
    """Conv2DTranspose: w_oihw [OC][IC][k][k]; output s*H ("same") or s*H + k - s (deconv2dGL.cpp:345-355)."""
    w = _f32(w_oihw)
    OC, IC, k, _ = w.shape
    p = (k - stride) // 2 if same else 0
    OH, OW = (stride * H, stride * W) if same else (stride * H + k - stride, stride * W + k - stride)
    d = _conv_desc(N, H, W, IC, OC, k, stride, (p, 0, 0, 0), "constant", act, leaky, bias is not None, bn is not None, OH, OW)
    b = _f32(bias) if bias is not None else None
    bnp = [_f32(bn[key]) for key in ("beta", "gamma", "mean", "var")] if bn is not None else [None] * 4
    h = _P()
    check(lib().snnhip_deconv2d_plan_create(ctx.h, C.byref(d), _fptr(w), _fptr(b), *[_fptr(a) for a in bnp], C.byref(h)))
    return Plan(ctx, h)


def espcn_f16_pack_weights(w_oihw, r=0):
    """snnhip_espcn_f16_pack_weights (host side only, no GPU): the lane-ordered fp16 image that the fp16 ESPCN kernels keep of a convolution's weights, as
    float16.  w_oihw [16][1][k][k] (k = 3, 5) or [OC][16][3][3] with r = 0 (OC = 16: MFMA row = channel) or r = 2, 3, 4 (OC = r*r: row 4*dy + dx)."""
    w = np.ascontiguousarray(w_oihw, dtype=np.float32)
    out = np.zeros(2304, np.uint16)
    n = C.c_int(0)
    check(lib().snnhip_espcn_f16_pack_weights(w.ctypes.data_as(_P), w.shape[1], w.shape[2], r, out.ctypes.data_as(_P), out.size, C.byref(n)))
    return out[: n.value].view(np.float16).copy()


def espcn_f16_wide_pack_weights(w_oihw, r=0):
    """snnhip_espcn_f16_wide_pack_weights (host side only, no GPU): the lane-ordered fp16 images of the fp16 ESPCN kernels at the published widths, as
    float16.  w_oihw [64][1][k][k] (k = 3, 5), [32][64][3][3] with r = 0 (MFMA row = channel) or [r*r][32][3][3] with r = 2, 3, 4 (row 4*dy + dx)."""
    w = np.ascontiguousarray(w_oihw, dtype=np.float32)
    out = np.zeros(18432, np.uint16)
    n = C.c_int(0)
    check(lib().snnhip_espcn_f16_wide_pack_weights(w.ctypes.data_as(_P), w.shape[0], w.shape[1], w.shape[2], r, out.ctypes.data_as(_P), out.size, C.byref(n)))
    return out[: n.value].view(np.float16).copy()


def chain_plan(ctx, plans):
    arr = (_P * len(plans))(*[p.h for p in plans])
    h = _P()
    check(lib().snnhip_chain_plan_create(ctx.h, arr, len(plans), C.byref(h)))
    return Plan(ctx, h, keep=tuple(plans))


def graph_fuse(ctx, nodes):
    """snnhip_graph_fuse: nodes = [(Plan, [producer index | -(k+1) for model input k], keep)] in execution order.
    Returns [(Plan | None, inputs)] per node: None = folded into a later node's plan, the same Plan object = unchanged, a new Plan = fused."""
    n = len(nodes)
    arr = (GraphNode * n)()
    for i, (plan, ins, keep) in enumerate(nodes):
        arr[i].plan = plan.h if plan is not None else None
        arr[i].n_inputs = len(ins)
        for k, v in enumerate(ins):
            arr[i].inputs[k] = v
        arr[i].keep = int(bool(keep))
    out = (FusedNode * n)()
    check(lib().snnhip_graph_fuse(ctx.h, arr, n, out))
    res = []
    for i, (plan, ins, _) in enumerate(nodes):
        o = out[i]
        if not o.plan:
            res.append((None, []))
        elif o.owned:
            res.append((Plan(ctx, _P(o.plan), keep=tuple(q for q, _, _ in nodes)), [o.inputs[k] for k in range(o.n_inputs)]))  # fused plans borrow their members
        else:
            res.append((plan, [o.inputs[k] for k in range(o.n_inputs)]))  # the node's own plan, possibly re-wired past a folded identity producer
    return res


class Graph:
    """A captured launch sequence (hipGraph): `with Graph.capture(ctx) as g: runner.run_device()`, then g.launch() replays it."""

    def __init__(self, ctx):
        self.ctx, self.h = ctx, _P()

    class _Cap:
        def __init__(self, g):
            self.g = g

        def __enter__(self):
            check(lib().snnhip_graph_begin_capture(self.g.ctx.h))
            return self.g

        def __exit__(self, et, ev, tb):
            rc = lib().snnhip_graph_end_capture(self.g.ctx.h, C.byref(self.g.h))
            if et is None:
                check(rc)
            return False

    @staticmethod
    def capture(ctx):
        return Graph._Cap(Graph(ctx))

    def launch(self):
        check(lib().snnhip_graph_launch(self.h))

    def num_nodes(self):
        return lib().snnhip_graph_num_nodes(self.h)

    def destroy(self):
        if self.h:
            lib().snnhip_graph_destroy(self.h)
            self.h = _P()


class Timer:
    def __init__(self, ctx):
        self.h = _P()
        check(lib().snnhip_timer_create(ctx.h, C.byref(self.h)))

    def start(self):
        check(lib().snnhip_timer_start(self.h))

    def stop(self):
        check(lib().snnhip_timer_stop(self.h))

    def elapsed_ms(self):
        ms = C.c_float()
        check(lib().snnhip_timer_elapsed_ms(self.h, C.byref(ms)))
        return ms.value

    def destroy(self):
        if self.h:
            lib().snnhip_timer_destroy(self.h)
            self.h = None
