"""ctypes binding of include/snn_c.h (libsnn_core.so): the C++ host mirror of the reference's MixedInferenceCore API."""
import ctypes as C
import os

import numpy as np

from . import capi

# SNN_CORE_LIB_PATH: another build of the host library (tools/sanitize.sh points it at lib/libsnn_core_asan.so)
LIB_PATH = os.environ.get("SNN_CORE_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libsnn_core.so")
_lib = None
_P = C.c_void_p
_FP = C.POINTER(C.c_float)

SIGNATURES = {
    "snn_model_create": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "snn_model_create2": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "snn_model_create3": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "snn_model_create4": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "snn_model_create5": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    "snn_model_create6": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    "snn_model_create7": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    "snn_model_create8": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    "snn_model_create9": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    "snn_model_create10": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    "snn_model_create11": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    "snn_model_create12": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    "snn_model_create13": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    "snn_model_create14": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    "snn_model_download_input": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "snn_model_upload_frame_planes": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int]),
    "snn_model_download_frame_planes": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int]),
    "snn_model_upload_frame_nv12": (C.c_int, [_P, _P]),
    "snn_model_download_frame_nv12": (C.c_int, [_P, _P]),
    "snn_model_upload_frame_u16": (C.c_int, [_P, _P]),
    "snn_model_download_frame_u16": (C.c_int, [_P, _P]),
    "snn_model_upload_frame_u8": (C.c_int, [_P, _P]),
    "snn_model_download_frame_u8": (C.c_int, [_P, _P]),
    "snn_model_reference_frame": (C.c_int, [_P, _P]),
    "snn_model_reference_frame_planes": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int]),
    "snn_model_frame_metrics": (C.c_int, [_P, _P, C.c_int]),
    "snn_model_batch": (C.c_int, [_P]),
    "snn_model_hip_ctx": (_P, [_P]),
    "snn_model_output_tensor": (_P, [_P]),
    "snn_pool_create": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "snn_pool_destroy": (C.c_int, [_P]),
    "snn_pool_replicas": (C.c_int, [_P]),
    "snn_pool_shard": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "snn_pool_output_dims": (C.c_int, [_P, C.POINTER(C.c_int * 3)]),
    "snn_pool_upload_input": (C.c_int, [_P, _FP]),
    "snn_pool_run": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double)]),
    "snn_pool_download_output": (C.c_int, [_P, _FP]),
    "snn_pool_allgather_output_rccl": (C.c_int, [_P, _FP]),
    "snn_model_stage_plan_steps": (C.c_int, [_P, C.c_int]),
    "snn_model_stage_plan_step": (C.c_int, [_P, C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "snn_model_profile_enable": (C.c_int, [_P, C.c_int]),
    "snn_model_profile_read": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "snn_model_suspend_replay": (C.c_int, [_P, C.c_int]),
    "snn_model_cost": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "snn_model_destroy": (C.c_int, [_P]),
    "snn_model_upload_input": (C.c_int, [_P, _FP]),
    "snn_model_run": (C.c_int, [_P]),
    "snn_model_run_async": (C.c_int, [_P]),
    "snn_model_sync": (C.c_int, [_P]),
    "snn_model_output_dims": (C.c_int, [_P, C.POINTER(C.c_int * 3)]),
    "snn_model_download_output": (C.c_int, [_P, _FP]),
    "snn_model_set_type": (C.c_int, [_P, C.c_int]),
    "snn_model_classifier_output": (C.c_int, [_P]),
    "snn_model_detections": (C.c_int, [_P, _FP, C.c_int]),
    "snn_model_upload_input_u8": (C.c_int, [_P, C.c_void_p, C.c_int, C.c_int, C.c_int, _FP, _FP, _FP, _FP]),
    "snn_yolo_decode": (C.c_int, [_FP, _FP, C.c_int, _FP, C.c_int]),
    "snn_model_num_stages": (C.c_int, [_P]),
    "snn_model_stage_info": (C.c_int, [_P, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int * 3), C.POINTER(C.c_int)]),
    "snn_model_download_stage": (C.c_int, [_P, C.c_int, _FP]),
    "snn_model_describe": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "snn_model_time_stats": (C.c_int, [_P, C.c_char_p, C.c_int, C.POINTER(C.c_double), C.c_int]),
    "snn_conv_test_with_layer": (C.c_int, [C.c_int, _FP, _FP, _FP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _FP, _FP, _FP, _FP,
                                           C.c_char_p, C.c_int]),
    "snn_graph_summary": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]),
    "snn_json_number": (C.c_int, [C.c_char_p, C.POINTER(C.c_double)]),
    "snn_model_create15": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    "snn_frames_resolve": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]),
    "snn_dump_read": (C.c_int, [C.c_char_p, C.POINTER(C.c_int * 4), _FP, C.c_long]),
}


class FrameMetrics(C.Structure):  # snn_frame_metrics
    _fields_ = [("image", C.c_int), ("plane", C.c_int), ("channel", C.c_int), ("sse", C.c_ulonglong), ("pixels", C.c_ulonglong), ("psnr_db", C.c_double),
                ("ssim", C.c_double)]


def lib():
    global _lib
    if _lib is None:
        capi.load_library()  # libsnnhip.so first (libsnn_core.so links against it)
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: run __graft_entry__.build()" % LIB_PATH)
        l = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def _fp(a):
    return None if a is None else a.ctypes.data_as(_FP)


def graph_summary(json_path, w, h, c):
    buf = C.create_string_buffer(1 << 16)
    n = lib().snn_graph_summary(json_path.encode(), w, h, c, buf, len(buf))
    if n < 0:  # the loader refused the model: buf holds its one-line reason
        raise ValueError("snn_graph_summary(%s) failed (%d): %s" % (json_path, n, buf.value.decode(errors="replace")))
    rows = []
    for line in buf.value.decode().strip().split("\n"):
        idx, name, loc, dims, ins = line.split("|")
        rows.append({"index": int(idx), "name": name, "loc": int(loc), "dims": tuple(int(v) for v in dims.split("x")),
                     "inputs": [int(v) for v in ins.split(",") if v]})
    assert len(rows) == n
    return rows


def json_number(text):
    """The model loader's JSON parser on one number literal (None if it refuses it)."""
    d = C.c_double()
    return d.value if lib().snn_json_number(text.encode(), C.byref(d)) == 0 else None


def frames_resolve(entry, io, w, h, c, batch=1):
    """The frame description snn_model_create<entry> resolves its struct `io` (None: a null struct) to, as one canonical line "<the model part> |
    <the frame ends> | entry=<name>"; None if the entry point refuses the request before it opens the model file.  Host-only."""
    buf = C.create_string_buffer(2048)
    rc = lib().snn_frames_resolve(entry, None if io is None else C.byref(io), w, h, c, batch, buf, len(buf))
    return buf.value.decode() if rc == 0 else None


def read_dump(path):
    """Reference .dump -> (W, H, D, C, float32 array [D][H][W][4])."""
    d = (C.c_int * 4)()
    assert lib().snn_dump_read(path.encode(), C.byref(d), None, 0) == 0
    w, h, dd, c = d
    out = np.empty((dd, h, w, 4), dtype=np.float32)
    assert lib().snn_dump_read(path.encode(), C.byref(d), _fp(out), out.size) == 0
    return w, h, dd, c, out


def c4hw4_to_nhwc(a, channels):
    d, h, w, _ = a.shape
    return np.transpose(a, (1, 2, 0, 3)).reshape(h, w, d * 4)[:, :, :channels]


def yolo_decode(head_coarse, head_fine, net_size=416, max_rows=100):
    """YOLOLayer's CPU decode + NMS (host-only)."""
    a, b = np.ascontiguousarray(head_coarse, dtype=np.float32), np.ascontiguousarray(head_fine, dtype=np.float32)
    rows = np.zeros((max_rows, 6), np.float32)
    n = lib().snn_yolo_decode(_fp(a), _fp(b), net_size, _fp(rows), max_rows)
    return rows[:n].copy()


class FrameIO(C.Structure):
    """snn_frame_io (include/snn_c.h): 8-bit frame formats at the model's ends and their affine maps."""
    _fields_ = [("in_format", C.c_int), ("out_format", C.c_int), ("in_means", C.c_float * 4), ("in_norms", C.c_float * 4), ("out_scale", C.c_float * 4),
                ("out_offset", C.c_float * 4)]


class FrameIO2(C.Structure):
    """snn_frame_io2 (include/snn_c.h): 8- or 16-bit frame formats at the model's ends, their affine maps and the 16-bit container layout."""
    _fields_ = FrameIO._fields_ + [("in_shift", C.c_int), ("out_maxval", C.c_int), ("out_shift", C.c_int)]


class ColourIO(C.Structure):
    """snn_colour_io (include/snn_c.h): RGB8 / RGBA8 frames around a luma-only model, the matrix coefficients and the luma plane's 8-bit maps."""
    _fields_ = [("format", C.c_int), ("kr", C.c_float), ("kb", C.c_float), ("in_mean", C.c_float), ("in_norm", C.c_float), ("out_scale", C.c_float),
                ("out_offset", C.c_float)]


class VideoIO(C.Structure):
    """snn_video_io (include/snn_c.h): NV12 / P010 frames around a luma-only model, the chroma plane's depth and siting and the luma plane's maps."""
    _fields_ = [("format", C.c_int), ("maxval", C.c_int), ("shift", C.c_int), ("siting", C.c_int), ("in_mean", C.c_float), ("in_norm", C.c_float),
                ("out_scale", C.c_float), ("out_offset", C.c_float)]


class FitIO(C.Structure):
    """snn_fit_io (include/snn_c.h): snn_video_io and the size the output frame is resampled to."""
    _fields_ = [("video", VideoIO), ("out_w", C.c_int), ("out_h", C.c_int)]


class VideoRgbIO(C.Structure):
    """snn_video_rgb_io (include/snn_c.h): NV12 / P010 frames in, RGB / RGBA frames out around a luma-only model; the luma maps follow from the range."""
    _fields_ = [("in_format", C.c_int), ("out_format", C.c_int), ("maxval", C.c_int), ("shift", C.c_int), ("siting", C.c_int), ("range", C.c_int),
                ("kr", C.c_float), ("kb", C.c_float)]


class EncodeIO(C.Structure):
    """snn_encode_io (include/snn_c.h): RGB8 / RGBA8 frames in, an NV12 frame out around a luma-only model; the luma maps follow from the range."""
    _fields_ = [("in_format", C.c_int), ("out_format", C.c_int), ("siting", C.c_int), ("range", C.c_int), ("kr", C.c_float), ("kb", C.c_float)]


class PlanarIO(C.Structure):
    """snn_planar_io (include/snn_c.h): planar 4:2:0 frames (I420 / I010) in and out around a luma-only model; the luma maps follow from the range."""
    _fields_ = [("in_format", C.c_int), ("out_format", C.c_int), ("maxval", C.c_int), ("shift", C.c_int), ("siting", C.c_int), ("range", C.c_int),
                ("kr", C.c_float), ("kb", C.c_float), ("out_w", C.c_int), ("out_h", C.c_int)]


class RgbFitIO(C.Structure):
    """snn_rgb_fit_io (include/snn_c.h): video or colour frames in, an RGB / RGBA frame at out_w x out_h out around a luma-only model."""
    _fields_ = [("in_format", C.c_int), ("out_format", C.c_int), ("maxval", C.c_int), ("shift", C.c_int), ("siting", C.c_int), ("range", C.c_int),
                ("kr", C.c_float), ("kb", C.c_float), ("out_w", C.c_int), ("out_h", C.c_int)]


class VideoTensorIO(C.Structure):
    """snn_video_tensor_io (include/snn_c.h): a 4:2:0 video frame of src_w x src_h in front of an RGB(A) model, straight to its normalised input tensor."""
    _fields_ = [("in_format", C.c_int), ("out_format", C.c_int), ("src_w", C.c_int), ("src_h", C.c_int), ("maxval", C.c_int), ("shift", C.c_int), ("siting", C.c_int),
                ("range", C.c_int), ("kr", C.c_float), ("kb", C.c_float), ("filter", C.c_int), ("means", C.c_float * 4), ("norms", C.c_float * 4), ("alpha", C.c_float),
                ("out_scale", C.c_float * 4), ("out_offset", C.c_float * 4)]


class TensorVideoIO(C.Structure):
    """snn_tensor_video_io (include/snn_c.h): the output tensor of an RGB(A) model to the planes of a 4:2:0 frame of the same extent; video_in as
    snn_model_create14 takes it when a video frame goes in."""
    _fields_ = [("in_format", C.c_int), ("out_format", C.c_int), ("maxval", C.c_int), ("shift", C.c_int), ("siting", C.c_int), ("range", C.c_int), ("kr", C.c_float),
                ("kb", C.c_float), ("out_scale", C.c_float * 4), ("out_offset", C.c_float * 4), ("in_means", C.c_float * 4), ("in_norms", C.c_float * 4),
                ("video_in", VideoTensorIO)]


VIDEO_FILTERS = {"nearest": 0, "linear": 1}  # SNN_FILTER_*
# name: (SNN_IO_NV12 / SNN_IO_NV12_16 / SNN_IO_I420 / SNN_IO_I420_16, maxval, shift); I010 is ffmpeg's yuv420p10le: 10 bits in the low end of 2 bytes
VIDEO_FORMATS = {"NV12": (0x201, 255, 0), "P010": (0x301, 1023, 6), "I420": (0x401, 255, 0), "I010": (0x501, 1023, 0)}
PLANAR_FORMATS = ("I420", "I010")
SITINGS = {"centre": 0, "left": 1}  # SNN_SITING_*
VIDEO_RANGES = {"limited": 0, "full": 1}  # SNN_RANGE_*
VIDEO_OUT_FORMATS = {"RGB8": (0x201, 3), "RGBA8": (0x201, 4), "RGB16": (0x301, 3), "RGBA16": (0x301, 4)}  # name: (the input format it pairs with, channels)
FRAME_FORMATS = {None: 0, "float": 0, "R8": 1, "RGB8": 3, "RGBA8": 4, "R16": 0x101, "RGB16": 0x103, "RGBA16": 0x104}  # SNN_IO_*


class Model:
    """MixedInferenceCore::create(context, jsonFile, options) + run(), one W x H x C input image."""

    def __init__(self, json_path, w, h, c, device=0, dump_outputs=False, fuse_chains=True, profiling=False, prefer_half=False, capture_graph=False,
                 batch=1, input_format=None, output_format=None, in_means=(0, 0, 0, 0), in_norms=(1, 1, 1, 1), out_scale=(1, 1, 1, 1),
                 out_offset=(0, 0, 0, 0), frame_in_shift=0, frame_out_maxval=65535, frame_out_shift=0, colour=None, kr=0.299, kb=0.114, video=None,
                 siting="left", video_maxval=None, video_shift=None, video_out=None, video_range="limited", out_size=None, rgb_size=None, frame_size=None,
                 video_filter="linear", alpha=1.0, encode=None, encode_maxval=None, encode_shift=None):
        """batch > 1: every stage tensor carries `batch` images (snn_model_create4); upload() takes and output() returns a leading batch axis.
        input_format / output_format "R8" / "RGB8" / "RGBA8": 8-bit frames at that end (snn_model_create5): upload_frame(uint8) feeds the input,
        output_frame() returns the uint8 output; y = (u - in_means[c]) * in_norms[c] in, clamp(rint(x * out_scale[c] + out_offset[c]), 0, 255) out.
        "R16" / "RGB16" / "RGBA16": 16-bit frames (snn_model_create6), uint16 arrays; y = ((u >> frame_in_shift) - in_means[c]) * in_norms[c] in,
        clamp(rint(x * out_scale[c] + out_offset[c]), 0, frame_out_maxval) << frame_out_shift out (10-bit: maxval 1023; P010-style: shifts 6).
        colour "RGB8" / "RGBA8" (snn_model_create7): colour frames around a luma-only model (c == 1, e.g. ESPCN) -- upload_frame takes uint8
        [batch x] H x W x C, output_frame returns [batch x] rH x rW x C: the model runs on the frame's luma plane (coefficients kr, kb; BT.601 by
        default) with R8 frames at its own ends (in_means[0] / in_norms[0] / out_scale[0] / out_offset[0]), the chroma is upsampled bicubically.
        video "NV12" / "P010" (snn_model_create8): a decoder's 4:2:0 frames around a luma-only model -- upload_frame takes a pair (y, cbcr) of uint8
        (uint16 for P010) arrays [batch x] H x W and [batch x] H/2 x W/2 x 2, output_frame / download_frame return the pair at r times the extent;
        the luma plane runs through the model with R8 / R16 frames at its ends, the chroma plane through one more launch (siting "left": co-sited
        with even luma columns, the default of H.264 / HEVC / AV1; "centre": JPEG / MPEG-1).  video_maxval / video_shift override the format's depth
        (P010: 1023, 6; low-aligned 12-bit would be 4095, 0).
        video_out "RGB8" / "RGBA8" (with "NV12") or "RGB16" / "RGBA16" (with "P010") beside video (snn_model_create9): the frames go in as above and
        come back as packed full-range RGB -- output_frame / download_frame return uint8 / uint16 [batch x] rH x rW x C.  video_range "limited" /
        "full" is the stream's range and sets the luma plane's maps (in_means / in_norms / out_scale / out_offset are not used); kr, kb are the
        stream's matrix (BT.601 by default, BT.709 is 0.2126 / 0.0722).  One launch behind the model's two converts: no chroma_up launch.
        colour "RGB8" / "RGBA8" with video_out "NV12" (snn_model_create10): capture in, encoder out -- upload_frame takes the uint8 RGB frame
        [batch x] H x W x C, output_frame / download_frame return the pair (y, cbcr) of the NV12 frame at r times the extent (r = 2..4, rH and rW
        even): y from the model (video_range sets its output map: "limited" 16 + 219 x, "full" 255 x), cbcr [batch x] rH/2 x rW/2 x 2 from the
        RGB frame in one launch behind the model (siting, kr, kb as above).  in_means / in_norms / out_scale / out_offset are not used.
        out_size (w, h) beside video alone (snn_model_create11): the NV12 / P010 frame comes back at that size, both even, between half and all of
        r times the input on each axis -- the model's luma frame and the original chroma plane resampled on the device, two launches behind the
        model's (no chroma launch); output_frame / download_frame return the pair (y, cbcr) at h x w and h/2 x w/2.
        video "I420" / "I010" (snn_model_create12): planar 4:2:0 frames, what software decoders and encoders use -- everything above for "NV12" /
        "P010" with the triple (y, cb, cr) in place of the pair: alone (the same planar format comes back), with out_size, with video_out "RGB8" /
        "RGBA8" ("I420") or "RGB16" / "RGBA16" ("I010"); and colour "RGB8" / "RGBA8" with video_out "I420".  video_range sets the luma plane's maps on
        every one of them (in_means / in_norms / out_scale / out_offset are not used).  upload_planes / download_planes take arrays with a row pitch.
        rgb_size (w, h) beside video and video_out "RGB8" / ... , or beside colour "RGB8" / "RGBA8" alone (snn_model_create13): the RGB frame comes
        back at that size (it need not be even), between half and all of r times the input on each axis and, with colour, no smaller than the
        input -- the model's luma frame resampled to the size, then RGB from it and the ORIGINAL chroma planes (or the colour frame that went in)
        in one more launch; no r-fold chroma or RGB frame is formed.  With colour the luma maps are 0, 1 / 255, 255, 0 (in_means / ... are not used).
        frame_size (src_w, src_h) beside video "NV12" / "P010" / "I420" / "I010" (snn_model_create14): video in front of an RGB(A) model -- w, h, c are
        the MODEL's input, c = 3 or 4, and a frame of that (even) size goes straight to the model's normalised input tensor in one launch:
        t = (sample - in_means[c]) * in_norms[c] with the sample in 0 .. maxval, channel 3 = alpha, video_filter "linear" / "nearest", siting,
        video_range, kr, kb the stream's.  upload_frame / upload_planes take the planes at frame_size; upload() and upload_u8() are refused;
        input_tensor() returns what the launch wrote.  output_format "RGB8" / ... (with out_scale / out_offset) makes the model's output an 8-bit
        frame as snn_model_create5 does; otherwise output() returns floats.
        encode "NV12" / "P010" / "I420" / "I010" (snn_model_create15): an encoder's frame behind an RGB(A) model -- the model's output tensor (3 or 4
        channels, an even extent) leaves as the planes of a 4:2:0 frame of its own extent in one launch behind the model:
        p = clamp(x * out_scale[c] + out_offset[c], 0, maxval) is full-range RGB at the output depth (encode_maxval / encode_shift override the
        format's: P010 1023, 6), siting, video_range, kr, kb the OUTPUT stream's.  It goes beside nothing (upload() takes floats), beside
        input_format "RGB8" / "RGBA8" (upload_frame takes uint8, in_means / in_norms), or beside video=..., frame_size=... (video in as above AND out:
        the stream's parameters serve both ends).  output_frame / download_frame return the pair (y, cbcr) or the triple (y, cb, cr),
        download_planes fills pitched planes; output() and the 8-bit downloads are refused."""
        self.h = _P()
        self.batch = batch
        self.video = video  # the upload end: None = one array (the model's frame or a colour frame), else planes of this format
        self.out_end = "frame"  # what comes back: "frame" = one array of out_channels (0: the model's own), "yuv" = luma + chroma planes
        self.out_channels = 0
        self.out_size = None
        self.frame_hw = None  # the extent of the planes that go in, where it is not the model input's (frame_size)
        in_channels, u8 = c, (np.uint8, np.uint8)
        if frame_size is not None:
            assert video in VIDEO_FORMATS, "frame_size is the size of a video frame: it goes with video=\"NV12\" / \"P010\" / \"I420\" / \"I010\""
            assert video_out is None and colour is None and out_size is None and rgb_size is None and input_format is None, \
                "frame_size puts video in front of an RGB model: not beside video_out / colour / out_size / rgb_size / input_format"
            assert output_format in (None, "float", "R8", "RGB8", "RGBA8"), "the model's output is float or an 8-bit frame"
            assert c in (3, 4), "the model takes 3 (RGB) or 4 (RGB + alpha) input channels"
            assert video_range in VIDEO_RANGES, "video_range is \"limited\" or \"full\""
            assert siting in SITINGS, "siting is \"left\" or \"centre\""
            assert video_filter in VIDEO_FILTERS, "video_filter is \"linear\" or \"nearest\""
            assert kr > 0 and kb > 0 and kr + kb < 1, "0 < kr, 0 < kb, kr + kb < 1"
            sw, sh = int(frame_size[0]), int(frame_size[1])
            assert sw >= 2 and sh >= 2 and sw % 2 == 0 and sh % 2 == 0, "a 4:2:0 frame has an even extent"
            fmt, maxval, shift = VIDEO_FORMATS[video]
            maxval = maxval if video_maxval is None else video_maxval
            shift = shift if video_shift is None else video_shift
            self.frame_hw = (sh, sw)
            self.frame_dtypes = (np.uint16 if fmt in (0x301, 0x501) else np.uint8, np.uint8)
            maps = [(C.c_float * 4)(*(tuple(m) + (0,) * 4)[:4]) for m in (in_means, in_norms, out_scale, out_offset)]
            tensor_io = VideoTensorIO(fmt, FRAME_FORMATS[output_format], sw, sh, maxval, shift, SITINGS[siting], VIDEO_RANGES[video_range], kr, kb, VIDEO_FILTERS[video_filter],
                                      maps[0], maps[1], alpha, maps[2], maps[3])
            video_out = colour = None
        if encode is not None:
            assert encode in VIDEO_FORMATS, "encode is \"NV12\", \"P010\", \"I420\" or \"I010\""
            assert video_out is None and colour is None and out_size is None and rgb_size is None and output_format is None, \
                "encode makes the output a 4:2:0 frame: not beside video_out / colour / out_size / rgb_size / output_format"
            assert (video is None) == (frame_size is None), "video frames in front of encode= need video= and frame_size= together"
            assert input_format in (None, "float", "RGB8", "RGBA8") and (input_format in (None, "float") or video is None), \
                "encode goes beside nothing, beside input_format=\"RGB8\" / \"RGBA8\", or beside video= and frame_size="
            assert video_range in VIDEO_RANGES, "video_range is \"limited\" or \"full\""
            assert siting in SITINGS, "siting is \"left\" or \"centre\""
            assert kr > 0 and kb > 0 and kr + kb < 1, "0 < kr, 0 < kb, kr + kb < 1"
            efmt, emaxval, eshift = VIDEO_FORMATS[encode]
            emaxval = emaxval if encode_maxval is None else encode_maxval
            eshift = eshift if encode_shift is None else encode_shift
            maps = [(C.c_float * 4)(*(tuple(m) + (0,) * 4)[:4]) for m in (out_scale, out_offset, in_means, in_norms)]
            encode_io = TensorVideoIO(fmt if video is not None else FRAME_FORMATS[input_format], efmt, emaxval, eshift, SITINGS[siting], VIDEO_RANGES[video_range], kr, kb, *maps,
                                      tensor_io if video is not None else VideoTensorIO())
            self.frame_dtypes = (self.frame_dtypes[0] if video is not None else np.uint8, np.uint16 if efmt in (0x301, 0x501) else np.uint8)
            self.out_end = "yuv"
        assert out_size is None or (video is not None and video_out is None and colour is None), "out_size fits an NV12 / P010 frame: it goes with video= alone"
        if encode is not None:
            entry, io = 15, encode_io
        elif frame_size is not None:
            entry, io = 14, tensor_io
        elif rgb_size is not None:
            assert out_size is None and input_format is None and output_format is None, "rgb_size is the size of an RGB frame: not beside out_size / input_format / output_format"
            assert (video is not None and video_out in VIDEO_OUT_FORMATS and colour is None) or (colour in ("RGB8", "RGBA8") and video is None and video_out is None), \
                "rgb_size goes with video= and video_out=\"RGB8\" / \"RGBA8\" / \"RGB16\" / \"RGBA16\", or with colour=\"RGB8\" / \"RGBA8\" alone"
            assert kr > 0 and kb > 0 and kr + kb < 1, "0 < kr, 0 < kb, kr + kb < 1"
            size = self.out_size = (int(rgb_size[0]), int(rgb_size[1]))
            if colour is not None:
                in_channels = self.out_channels = {"RGB8": 3, "RGBA8": 4}[colour]
                self.frame_dtypes = u8
                io = RgbFitIO(FRAME_FORMATS[colour], FRAME_FORMATS[colour], 255, 0, SITINGS["centre"], VIDEO_RANGES["full"], kr, kb, *size)
            else:
                assert video_range in VIDEO_RANGES, "video_range is \"limited\" or \"full\""
                assert siting in SITINGS, "siting is \"left\" or \"centre\""
                fmt, maxval, shift = VIDEO_FORMATS[video]
                pair, self.out_channels = VIDEO_OUT_FORMATS[video_out]
                wide = fmt in (0x301, 0x501)
                assert pair == (0x301 if wide else 0x201), "%s frames come back as %s" % (video, "RGB16 / RGBA16" if wide else "RGB8 / RGBA8")
                maxval = maxval if video_maxval is None else video_maxval
                shift = shift if video_shift is None else video_shift
                in_channels, self.frame_dtypes = 1, ((np.uint16, np.uint16) if wide else u8)
                io = RgbFitIO(fmt, FRAME_FORMATS[video_out], maxval, shift, SITINGS[siting], VIDEO_RANGES[video_range], kr, kb, *size)
            entry = 13
        elif colour is not None and video_out is not None:
            assert video is None, "colour frames go in: video= names NV12 / P010 frames at the input"
            assert colour in ("RGB8", "RGBA8"), "colour is \"RGB8\" or \"RGBA8\""
            assert video_out in ("NV12", "I420"), "a colour frame leaves as video_out=\"NV12\" or \"I420\""
            assert video_range in VIDEO_RANGES, "video_range is \"limited\" or \"full\""
            assert siting in SITINGS, "siting is \"left\" or \"centre\""
            assert input_format is None and output_format is None, "colour frames replace input_format / output_format"
            assert kr > 0 and kb > 0 and kr + kb < 1, "0 < kr, 0 < kb, kr + kb < 1"
            in_channels, self.frame_dtypes, self.out_end = {"RGB8": 3, "RGBA8": 4}[colour], u8, "yuv"
            if video_out == "I420":
                entry, io = 12, PlanarIO(FRAME_FORMATS[colour], VIDEO_FORMATS["I420"][0], 255, 0, SITINGS[siting], VIDEO_RANGES[video_range], kr, kb, 0, 0)
            else:
                entry, io = 10, EncodeIO(FRAME_FORMATS[colour], VIDEO_FORMATS["NV12"][0], SITINGS[siting], VIDEO_RANGES[video_range], kr, kb)
        elif video_out is not None:
            assert video is not None, "video_out needs video=\"NV12\" or \"P010\""
            assert video_out in VIDEO_OUT_FORMATS, "video_out is one of %s" % sorted(VIDEO_OUT_FORMATS)
            assert video_range in VIDEO_RANGES, "video_range is \"limited\" or \"full\""
            assert siting in SITINGS, "siting is \"left\" or \"centre\""
            assert input_format is None and output_format is None and colour is None, "video frames replace input_format / output_format / colour"
            fmt, maxval, shift = VIDEO_FORMATS[video]
            pair, self.out_channels = VIDEO_OUT_FORMATS[video_out]
            wide = fmt in (0x301, 0x501)
            assert pair == (0x301 if wide else 0x201), "%s frames come back as %s" % (video, "RGB16 / RGBA16" if wide else "RGB8 / RGBA8")
            assert kr > 0 and kb > 0 and kr + kb < 1, "0 < kr, 0 < kb, kr + kb < 1"
            maxval = maxval if video_maxval is None else video_maxval
            shift = shift if video_shift is None else video_shift
            in_channels, self.frame_dtypes = 1, ((np.uint16, np.uint16) if wide else u8)
            if video in PLANAR_FORMATS:
                entry, io = 12, PlanarIO(fmt, FRAME_FORMATS[video_out], maxval, shift, SITINGS[siting], VIDEO_RANGES[video_range], kr, kb, 0, 0)
            else:
                entry, io = 9, VideoRgbIO(fmt, FRAME_FORMATS[video_out], maxval, shift, SITINGS[siting], VIDEO_RANGES[video_range], kr, kb)
        elif video is not None:
            assert input_format is None and output_format is None and colour is None, "video frames replace input_format / output_format / colour"
            fmt, maxval, shift = VIDEO_FORMATS[video]
            maxval = maxval if video_maxval is None else video_maxval
            shift = shift if video_shift is None else video_shift
            in_channels, self.frame_dtypes, self.out_end = 1, ((np.uint16, np.uint16) if fmt in (0x301, 0x501) else u8), "yuv"
            size = self.out_size = (int(out_size[0]), int(out_size[1])) if out_size is not None else None
            if video in PLANAR_FORMATS:
                assert video_range in VIDEO_RANGES, "video_range is \"limited\" or \"full\""
                assert siting in SITINGS, "siting is \"left\" or \"centre\""
                entry, io = 12, PlanarIO(fmt, fmt, maxval, shift, SITINGS[siting], VIDEO_RANGES[video_range], kr, kb, *(size or (0, 0)))
            else:
                entry, io = 8, VideoIO(fmt, maxval, shift, SITINGS[siting], in_means[0], in_norms[0], out_scale[0], out_offset[0])
                if size is not None:
                    entry, io = 11, FitIO(io, *size)
        elif colour is not None:
            assert input_format is None and output_format is None, "colour frames replace input_format / output_format"
            in_channels = self.out_channels = {"RGB8": 3, "RGBA8": 4}[colour]
            self.frame_dtypes = u8
            entry, io = 7, ColourIO(FRAME_FORMATS[colour], kr, kb, in_means[0], in_norms[0], out_scale[0], out_offset[0])
        else:
            self.frame_dtypes = tuple(np.uint16 if f in ("R16", "RGB16", "RGBA16") else np.uint8 for f in (input_format, output_format))
            maps = [(C.c_float * 4)(*m) for m in (in_means, in_norms, out_scale, out_offset)]
            if np.uint16 in self.frame_dtypes:
                entry, io = 6, FrameIO2(FRAME_FORMATS[input_format], FRAME_FORMATS[output_format], *maps, frame_in_shift, frame_out_maxval, frame_out_shift)
            else:
                entry, io = 5, FrameIO(FRAME_FORMATS[input_format], FRAME_FORMATS[output_format], *maps)
        self.planar = entry == 12 or (entry in (13, 14, 15) and video in PLANAR_FORMATS)
        self.out_planar = encode in PLANAR_FORMATS if entry == 15 else self.planar  # the download end's layout: its own behind encode=
        self.in_shape = (h, w, in_channels) if batch == 1 else (batch, h, w, in_channels)
        create = getattr(lib(), "snn_model_create%d" % entry)
        assert create(json_path.encode(), device, w, h, c, int(dump_outputs), int(fuse_chains), int(profiling), int(prefer_half), int(capture_graph), int(batch),
                      C.byref(io), C.byref(self.h)) == 0

    def upload_frame(self, img):
        """uint8 (uint16 for a 16-bit input format) [batch x] H x W x C into the model's input frame (no per-call allocation)."""
        if self.video and self.planar:
            return self._upload_planar(*img)
        if self.video:
            return self._upload_video(*img)
        img = np.ascontiguousarray(img, dtype=self.frame_dtypes[0]).reshape(self.in_shape)
        up = lib().snn_model_upload_frame_u16 if self.frame_dtypes[0] == np.uint16 else lib().snn_model_upload_frame_u8
        assert up(self.h, img.ctypes.data_as(_P)) == 0

    def output_frame(self):
        """the model's output frame of the last run, uint8 (uint16 for a 16-bit output format) [batch x] H x W x C"""
        d = (C.c_int * 3)()
        lib().snn_model_output_dims(self.h, C.byref(d))
        if self.out_end == "yuv":
            oh, ow = (self.out_size[1], self.out_size[0]) if self.out_size is not None else (d[0], d[1])
            return self._download_planar(oh, ow) if self.out_planar else self._download_video(oh, ow)
        if self.out_size is not None:  # rgb_size: the RGB frame at that size
            d = (self.out_size[1], self.out_size[0], d[2])
        if self.out_channels:
            d = (d[0], d[1], self.out_channels)
        out = np.empty(tuple(d) if self.batch == 1 else (self.batch,) + tuple(d), dtype=self.frame_dtypes[1])
        down = lib().snn_model_download_frame_u16 if self.frame_dtypes[1] == np.uint16 else lib().snn_model_download_frame_u8
        assert down(self.h, out.ctypes.data_as(_P)) == 0
        return out

    download_frame = output_frame

    def _upload_video(self, y, cbcr):
        """(y, cbcr) -> `batch` frames, each the luma plane followed by the interleaved chroma plane, the layout snn_model_upload_frame_nv12 takes"""
        dt, n = self.frame_dtypes[0], self.batch
        h, w = self.frame_hw or (self.in_shape[-3], self.in_shape[-2])
        y = np.ascontiguousarray(y, dtype=dt).reshape(n, h * w)
        cbcr = np.ascontiguousarray(cbcr, dtype=dt).reshape(n, (h // 2) * w)
        frames = np.ascontiguousarray(np.concatenate([y, cbcr], axis=1))
        assert lib().snn_model_upload_frame_nv12(self.h, frames.ctypes.data_as(_P)) == 0

    def _download_video(self, oh, ow):
        dt, n = self.frame_dtypes[1], self.batch
        frames = np.empty((n, oh * ow + (oh // 2) * ow), dtype=dt)
        assert lib().snn_model_download_frame_nv12(self.h, frames.ctypes.data_as(_P)) == 0
        y = frames[:, :oh * ow].reshape(n, oh, ow)
        cbcr = frames[:, oh * ow:].reshape(n, oh // 2, ow // 2, 2)
        return (y[0].copy(), cbcr[0].copy()) if n == 1 else (y.copy(), cbcr.copy())

    def _plane_args(self, planes, dtype):
        """(pointer array, pitch array, n_planes) of snn_model_upload_frame_planes / _download_frame_planes from batch * n_planes 2-D arrays, frame
        by frame (Y, Cb, Cr; or Y, CbCr with the interleaved plane as rows of W elements): rows contiguous, strides[0] the pitch in bytes, the same
        for that plane of every frame."""
        planes = list(planes)
        assert planes and len(planes) % self.batch == 0, "batch * n_planes arrays, frame by frame"
        k = len(planes) // self.batch
        for a in planes:
            assert isinstance(a, np.ndarray) and a.ndim == 2 and a.dtype == dtype and a.strides[1] == a.itemsize and a.strides[0] >= 0, "2-D %s arrays with contiguous rows" % np.dtype(dtype).name
        pitches = [planes[p].strides[0] for p in range(k)]
        for i, a in enumerate(planes):
            assert a.strides[0] == pitches[i % k], "one pitch per plane, the same for every frame"
        return (C.c_void_p * len(planes))(*[a.ctypes.data for a in planes]), (C.c_int * k)(*pitches), k, planes

    def upload_planes(self, planes):
        """snn_model_upload_frame_planes: batch * n_planes 2-D arrays with any row pitch (views into wider buffers: ffmpeg's data[] / linesize[]),
        frame by frame -- Y, Cb, Cr on a planar end, Y, CbCr (rows of W interleaved elements) on an NV12 / P010 end.  Padding is never read."""
        ptrs, pitches, k, keep = self._plane_args(planes, self.frame_dtypes[0])
        assert lib().snn_model_upload_frame_planes(self.h, ptrs, pitches, k) == 0
        del keep

    def download_planes(self, planes):
        """snn_model_download_frame_planes into the caller's (writable) arrays, laid out as for upload_planes at the output's extent; only each
        row's own bytes are written."""
        ptrs, pitches, k, keep = self._plane_args(planes, self.frame_dtypes[1])
        assert all(a.flags.writeable for a in keep)
        assert lib().snn_model_download_frame_planes(self.h, ptrs, pitches, k) == 0

    def _upload_planar(self, y, cb, cr):
        """(y, cb, cr), [batch x] H x W and twice [batch x] H/2 x W/2 -> snn_model_upload_frame_planes with tight pitches"""
        dt, n = self.frame_dtypes[0], self.batch
        h, w = self.frame_hw or (self.in_shape[-3], self.in_shape[-2])
        y = np.ascontiguousarray(y, dtype=dt).reshape(n, h, w)
        cb = np.ascontiguousarray(cb, dtype=dt).reshape(n, h // 2, w // 2)
        cr = np.ascontiguousarray(cr, dtype=dt).reshape(n, h // 2, w // 2)
        self.upload_planes([a[i] for i in range(n) for a in (y, cb, cr)])

    def _download_planar(self, oh, ow):
        dt, n = self.frame_dtypes[1], self.batch
        y, cb, cr = np.empty((n, oh, ow), dt), np.empty((n, oh // 2, ow // 2), dt), np.empty((n, oh // 2, ow // 2), dt)
        self.download_planes([a[i] for i in range(n) for a in (y, cb, cr)])
        return (y[0], cb[0], cr[0]) if n == 1 else (y, cb, cr)

    def _output_extent(self):
        d = (C.c_int * 3)()
        lib().snn_model_output_dims(self.h, C.byref(d))
        return (self.out_size[1], self.out_size[0]) if self.out_size is not None else (d[0], d[1]), d[2]

    def set_reference(self, ref):
        """The ground-truth frame metrics() compares the output against, at the OUTPUT's extent, mirroring upload_frame / upload_planes: one array
        [batch x] H x W x C for a packed output frame (snn_model_reference_frame); the pair (y, cbcr) for an NV12 / P010 output, the triple (y, cb,
        cr) for a planar one; or batch * n_planes 2-D arrays with any row pitch, frame by frame, as upload_planes takes them
        (snn_model_reference_frame_planes).  Kept on the device; a later call replaces it."""
        dt, n = self.frame_dtypes[1], self.batch
        (oh, ow), oc = self._output_extent()
        if self.out_end != "yuv":
            assert isinstance(ref, np.ndarray), "a packed output frame takes one array [batch x] H x W x C"
            ref = np.ascontiguousarray(ref, dtype=dt)
            assert ref.size == n * oh * ow * (self.out_channels or oc), "the reference has the output frame's extent: %d x %d x %d" % (oh, ow, self.out_channels or oc)
            assert lib().snn_model_reference_frame(self.h, ref.ctypes.data_as(_P)) == 0, "snn_model_reference_frame refused (see the log)"
            return
        parts = list(ref)
        k = 3 if self.out_planar else 2
        if len(parts) == n * k and all(isinstance(a, np.ndarray) and a.ndim == 2 for a in parts):  # plane arrays, any pitch
            ptrs, pitches, k, keep = self._plane_args(parts, dt)
            assert lib().snn_model_reference_frame_planes(self.h, ptrs, pitches, k) == 0, "snn_model_reference_frame_planes refused (see the log)"
            del keep
            return
        assert len(parts) == k, "an %s output takes %s" % ("I420 / I010" if self.out_planar else "NV12 / P010", "(y, cb, cr)" if self.out_planar else "(y, cbcr)")
        if self.out_planar:
            y, cb, cr = (np.ascontiguousarray(a, dtype=dt).reshape(n, hh, ww) for a, (hh, ww) in zip(parts, ((oh, ow), (oh // 2, ow // 2), (oh // 2, ow // 2))))
            return self.set_reference([a[i] for i in range(n) for a in (y, cb, cr)])
        y = np.ascontiguousarray(parts[0], dtype=dt).reshape(n, oh * ow)
        cbcr = np.ascontiguousarray(parts[1], dtype=dt).reshape(n, (oh // 2) * ow)
        frames = np.ascontiguousarray(np.concatenate([y, cbcr], axis=1))
        assert lib().snn_model_reference_frame(self.h, frames.ctypes.data_as(_P)) == 0, "snn_model_reference_frame refused (see the log)"

    def metrics(self):
        """snn_model_frame_metrics: PSNR and SSIM of the last run's output frame against the reference, computed on the device.  One dict {image,
        plane, channel, sse, pixels, psnr_db, ssim} per (image, plane, channel), image-major; plane 0 is the frame (or its luma plane), a video
        output's chroma follows as plane 1 with channels 0 / 1 (NV12 / P010) or planes 1 / 2 (I420 / I010)."""
        cap = self.batch * 8
        rows = (FrameMetrics * cap)()
        n = lib().snn_model_frame_metrics(self.h, rows, cap)
        assert n >= 0, "snn_model_frame_metrics refused: no reference set, or the output is a float tensor (see the log)"
        return [{f: getattr(r, f) for f, _ in FrameMetrics._fields_} for r in rows[:n]]

    def input_tensor(self):
        """snn_model_download_input: the model's input tensor as float32 [batch x] H x W x C -- what the [yuv tensor] launch of a frame_size model wrote
        in the last run, or the last upload()."""
        out = np.empty(self.in_shape, np.float32)
        assert lib().snn_model_download_input(self.h, _fp(out)) == 0
        return out

    def upload(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(self.in_shape)
        assert lib().snn_model_upload_input(self.h, _fp(x)) == 0

    def upload_u8(self, img, means=(0, 0, 0, 0), norms=(1, 1, 1, 1), resize_means=(0, 0, 0, 0), resize_norms=(1, 1, 1, 1)):
        """8-bit H x W x {1,3,4} image -> normalise -> bilinear resize to the model input, all on the device (modelInference.cpp:92-97)."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        ih, iw, ic = img.shape
        arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in (means, norms, resize_means, resize_norms)]
        rc = lib().snn_model_upload_input_u8(self.h, img.ctypes.data_as(C.c_void_p), iw, ih, ic, *[_fp(a) for a in arrs])
        assert rc == 0, rc

    MODEL_TYPES = {"classification": 0, "detection": 1, "segmentation": 2, "other": 3}

    def set_type(self, model_type):
        assert lib().snn_model_set_type(self.h, self.MODEL_TYPES[model_type]) == 0

    def classifier_output(self):
        """1-based class index of the last run (MixedInferenceCore::run, core.cpp:228-234); 0 = none."""
        return lib().snn_model_classifier_output(self.h)

    def detections(self, max_rows=100):
        rows = np.zeros((max_rows, 6), np.float32)
        n = lib().snn_model_detections(self.h, _fp(rows), max_rows)
        return rows[:n].copy()

    def run(self):
        assert lib().snn_model_run(self.h) == 0

    def run_async(self):
        """RunParameters::deferSync: enqueue one inference, no wait (pair with sync())."""
        assert lib().snn_model_run_async(self.h) == 0

    def sync(self):
        assert lib().snn_model_sync(self.h) == 0

    def output(self):
        d = (C.c_int * 3)()
        lib().snn_model_output_dims(self.h, C.byref(d))
        out = np.empty(tuple(d) if self.batch == 1 else (self.batch,) + tuple(d), dtype=np.float32)
        assert lib().snn_model_download_output(self.h, _fp(out)) == 0
        return out

    def __call__(self, x):
        self.upload(x)
        self.run()
        return self.output()

    def stages(self):
        out = []
        for i in range(lib().snn_model_num_stages(self.h)):
            name = C.create_string_buffer(512)
            d = (C.c_int * 3)()
            fused = C.c_int()
            lib().snn_model_stage_info(self.h, i, name, 512, C.byref(d), C.byref(fused))
            out.append({"name": name.value.decode(), "hwc": tuple(d), "fused_away": bool(fused.value & 1), "side": bool(fused.value & 2), "group": bool(fused.value & 4)})
        return out

    def stage_output(self, i):
        st = self.stages()[i]
        out = np.empty(st["hwc"] if self.batch == 1 else (self.batch,) + tuple(st["hwc"]), dtype=np.float32)
        if lib().snn_model_download_stage(self.h, i, _fp(out)) != 0:
            return None
        return out

    def plan_steps(self):
        """[(stage, step, kernel description, flops, bytes)] of every kernel launch of one inference, after fusion."""
        out = []
        for i in range(lib().snn_model_num_stages(self.h)):
            for k in range(lib().snn_model_stage_plan_steps(self.h, i)):
                desc = C.create_string_buffer(1024)
                f, b = C.c_double(), C.c_double()
                assert lib().snn_model_stage_plan_step(self.h, i, k, desc, 1024, C.byref(f), C.byref(b)) == 0
                out.append((i, k, desc.value.decode(), f.value, b.value))
        return out

    def profile(self, enable=True):
        assert lib().snn_model_profile_enable(self.h, int(enable)) == 0

    def suspend_replay(self, suspend=True):
        """launch by launch instead of replaying the recorded hipGraph (a launch trace needs the plans to run)"""
        assert lib().snn_model_suspend_replay(self.h, int(suspend)) == 0

    def profile_read(self, stage, step):
        ms, n = C.c_double(), C.c_int()
        assert lib().snn_model_profile_read(self.h, stage, step, C.byref(ms), C.byref(n)) == 0
        return ms.value, n.value

    def cost(self):
        f, b = C.c_double(), C.c_double()
        assert lib().snn_model_cost(self.h, C.byref(f), C.byref(b)) == 0
        return f.value, b.value

    def describe(self):
        buf = C.create_string_buffer(1 << 14)
        lib().snn_model_describe(self.h, buf, len(buf))
        return buf.value.decode()

    def time_stats(self):
        names = C.create_string_buffer(1 << 14)
        ms = (C.c_double * 256)()
        n = lib().snn_model_time_stats(self.h, names, len(names), ms, 256)
        return dict(zip(names.value.decode().strip().split("\n"), list(ms)[:n]))

    def close(self):
        if self.h:
            lib().snn_model_destroy(self.h)
            self.h = None


def conv_test_with_layer(x_hwc, w_oihw, bias, stride=1, pad=0, bn=None, device=0):
    """ShaderUnitTest::snnConvTestWithLayer; returns the dump path written by the layer."""
    x = np.ascontiguousarray(x_hwc, dtype=np.float32)
    w = np.ascontiguousarray(w_oihw, dtype=np.float32)
    h, ww, ic = x.shape
    oc, _, k, _ = w.shape
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    arrs = [None] * 4
    if bn is not None:
        arrs = [np.ascontiguousarray(bn[q], dtype=np.float32) for q in ("gamma", "mean", "var", "beta")]
    path = C.create_string_buffer(1024)
    rc = lib().snn_conv_test_with_layer(device, _fp(x), _fp(w), _fp(b), ww, h, ic, oc, k, stride, pad, int(bn is not None), _fp(arrs[0]), _fp(arrs[1]),
                                        _fp(arrs[2]), _fp(arrs[3]), path, 1024)
    assert rc == 0
    return path.value.decode()


class Pool:
    """snn_pool (include/snn_c.h): one replica (host thread + HipContext + stream) per entry of `devices`, a global batch split [g*B/G, (g+1)*B/G)."""

    def __init__(self, json_path, w, h, c, devices, global_batch, micro_batch=0, prefer_half=False, capture_graph=True):
        self.h = _P()
        devs = (C.c_int * len(devices))(*devices)
        rc = lib().snn_pool_create(json_path.encode(), devs, len(devices), w, h, c, int(prefer_half), int(capture_graph), global_batch, micro_batch, C.byref(self.h))
        if rc != 0:
            raise RuntimeError("snn_pool_create failed: %d" % rc)
        self.global_batch, self.in_shape = global_batch, (global_batch, h, w, c)
        hwc = (C.c_int * 3)()
        lib().snn_pool_output_dims(self.h, C.byref(hwc))
        self.out_shape = (global_batch,) + tuple(hwc)

    def replicas(self):
        return lib().snn_pool_replicas(self.h)

    def shard(self, g):
        a, b, s = C.c_int(), C.c_int(), C.c_int()
        assert lib().snn_pool_shard(self.h, g, C.byref(a), C.byref(b), C.byref(s)) == 0
        return a.value, b.value, s.value

    def upload(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.shape == self.in_shape, (x.shape, self.in_shape)
        assert lib().snn_pool_upload_input(self.h, _fp(x)) == 0

    def run(self, steps=1):
        sec = C.c_double()
        rc = lib().snn_pool_run(self.h, steps, C.byref(sec))
        if rc != 0:
            raise RuntimeError("snn_pool_run failed: %d" % rc)
        return sec.value

    def output(self, rccl=False):
        out = np.empty(self.out_shape, dtype=np.float32)
        rc = (lib().snn_pool_allgather_output_rccl if rccl else lib().snn_pool_download_output)(self.h, _fp(out))
        if rc != 0:
            raise RuntimeError("snn_pool output gather failed: %d" % rc)
        return out

    def close(self):
        if self.h:
            lib().snn_pool_destroy(self.h)
            self.h = None
