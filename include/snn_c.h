/*
 * snn_c.h -- C binding of the C++ host mirror (shadernn_amd/host, libsnn_core.so) for tests and bench harnesses.
 *
 * This is NOT the drop-in boundary (that is snnhip.h).  It lets non-C++ callers (pytest via ctypes) drive the same call
 * sequence the reference's own harnesses use:
 *   MixedInferenceCore::create(context, jsonFile, ShaderGenOptions) + run(RunParameters)
 *       -- demo/common/inferenceProcessor.cpp:42-140
 *   ShaderUnitTest::snnConvTestWithLayer: hand-built InputLayer + Conv2D layer, generateInferenceGraph, create, run, read the
 *   "<layer name> pass[0].dump" file            -- demo/common/shaderUnitTest.cpp:174-280
 * All functions return 0 on success; the C++ side aborts (SNN_RIP) on fatal errors exactly like the reference.
 */
#ifndef SNN_C_H
#define SNN_C_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct snn_model snn_model;
struct snnhip_ctx;    /* include/snnhip.h */
struct snnhip_tensor;

/* Loads a JSON model, builds the graph for one W x H x C input image and initialises every stage on `device`.
 * dump_outputs: write "<SNN_OUTPUT_DIR>/<layer name> pass[0].dump" for every layer on each run (disables fusion).
 * fuse_chains : let the HIP backend replace linear runs of layers by fused kernels. */
int snn_model_create(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                     snn_model** out);
/* as snn_model_create, with the reference's preferHp / ShaderGenOptions::preferrHalfPrecision switch: RGBA16F textures (half tensors in HBM),
 * weights truncated to fp16 at parse time (convertToMediumPrecision), fp16-MFMA convolutions.  Layers without an fp16 kernel (depthwise,
 * dense) abort the run like an unsupported layer does in the reference. */
int snn_model_create2(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                      int prefer_half, snn_model** out);
/* as snn_model_create2, plus capture_graph: record the first run's launches as a hipGraph and replay it afterwards (ignored with dumps / profiling) */
int snn_model_create3(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                      int prefer_half, int capture_graph, snn_model** out);
/* as snn_model_create3, for a BATCH of `batch` images per inference: every stage tensor is [batch][H][W][C] (the reference fixes the 4th
 * texture dimension to 1, core/src/ic2/core.cpp:371; here it carries the image count).  Uploads / downloads move batch x H x W x C floats. */
int snn_model_create4(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                      int prefer_half, int capture_graph, int batch, snn_model** out);
/* 8-bit frames at the model's ends (the reference's InferenceGraph::IODesc::format / ShaderGenOptions::desiredOutputFormat = ColorFormat::R8,
 * RGB8 or RGBA8).  in_format / out_format: SNN_IO_FLOAT (the model's fp32 / fp16 tensors, as snn_model_create4) or an 8-bit format whose channel
 * count is the model input's / output's own.  The input frame is y = (u - in_means[c]) * in_norms[c], the output q = clamp(rint(fmaf(x,
 * out_scale[c], out_offset[c])), 0, 255) (include/snnhip.h, snnhip_u8_in_plan_create / _u8_out_plan_create); the conversions join the fusion
 * graph, so for ESPCN they run inside its two fused kernels. */
enum { SNN_IO_FLOAT = 0, SNN_IO_R8 = 1, SNN_IO_RGB8 = 3, SNN_IO_RGBA8 = 4 };
typedef struct snn_frame_io {
    int in_format, out_format;
    float in_means[4], in_norms[4];
    float out_scale[4], out_offset[4];
} snn_frame_io;
int snn_model_create5(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                      int prefer_half, int capture_graph, int batch, const snn_frame_io* io, snn_model** out);
/* [batch][H][W][C] bytes into the model's input frame / out of its output frame (after snn_model_run or snn_model_sync); no allocation per
 * call, the tensors are the model's own, so a recorded graph replays across calls.  -1 when the model has no 8-bit frame at that end. */
int snn_model_upload_frame_u8(snn_model* m, const unsigned char* nhwc);
int snn_model_download_frame_u8(snn_model* m, unsigned char* nhwc);
/* 16-bit frames at the model's ends (10 / 12 / 16-bit video in 2-byte containers): SNN_IO_R16 / RGB16 / RGBA16 beside the formats above, through
 * a struct and an entry point of their own -- snn_frame_io and snn_model_create5 keep their layout and behaviour.  The input frame is
 * y = (float(u >> in_shift) - in_means[c]) * in_norms[c], the output q = unsigned(clamp(rint(fmaf(x, out_scale[c], out_offset[c])), 0,
 * out_maxval)) << out_shift (include/snnhip.h, snnhip_u16_in_plan_create / _u16_out_plan_create); the three fields are ignored at an end that is
 * not 16-bit.  Low-aligned 10 / 12-bit: out_maxval 1023 / 4095, shifts 0; P010-style high-aligned 10-bit: out_maxval 1023, shifts 6; full
 * 16-bit: out_maxval 65535.  For ESPCN in fp32 the conversions run inside its two fused kernels, as the 8-bit ones do. */
enum { SNN_IO_R16 = 0x101, SNN_IO_RGB16 = 0x103, SNN_IO_RGBA16 = 0x104 }; /* (low byte = channel count) */
typedef struct snn_frame_io2 {
    int in_format, out_format;
    float in_means[4], in_norms[4];
    float out_scale[4], out_offset[4];
    int in_shift, out_maxval, out_shift;
} snn_frame_io2;
int snn_model_create6(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                      int prefer_half, int capture_graph, int batch, const snn_frame_io2* io, snn_model** out);
/* [batch][H][W][C] 16-bit elements into the model's input frame / out of its output frame; -1 when that end is not a 16-bit frame (the _u8 calls
 * likewise return -1 on a 16-bit end). */
int snn_model_upload_frame_u16(snn_model* m, const unsigned short* nhwc);
int snn_model_download_frame_u16(snn_model* m, unsigned short* nhwc);
/* Colour frames around a luma-only model (ESPCN: one channel in, one channel out at r times the extent, r = 1..4): RGB8 or RGBA8 frames at BOTH ends,
 * through a struct and an entry point of their own -- snn_frame_io, snn_frame_io2 and snn_model_create5 / 6 keep their layout and behaviour (an RGB8
 * format on a one-channel model through them still returns -1).  The model itself is built exactly as snn_model_create5 builds it with SNN_IO_R8 at
 * both ends (in_mean / in_norm / out_scale / out_offset are the luma plane's u8_in / u8_out maps, so ESPCN still runs as its two fused 8-bit
 * kernels); a run brackets it with two more launches on the same stream: the colour frame's luma plane into the model's input frame
 * (snnhip_rgb_luma_plan_create), and the model's output frame merged with the colour frame's bicubically upsampled chroma into the colour output
 * frame (snnhip_ycc_merge_plan_create; include/snnhip.h states the arithmetic, kr / kb are its matrix coefficients: BT.601 0.299 / 0.114).  With
 * capture_graph all four launches are in the one recorded graph.  snn_model_upload_frame_u8 then takes [batch][H][W][C] bytes and
 * snn_model_download_frame_u8 returns [batch][rH][rW][C]; snn_model_describe lists the two extra launches.  Returns -1 unless the model has a
 * one-channel input and a one-channel output of r times the input's extent, r = 1..4, and format is SNN_IO_RGB8 or SNN_IO_RGBA8. */
typedef struct snn_colour_io {
    int format; /* SNN_IO_RGB8 or SNN_IO_RGBA8, both ends */
    float kr, kb;
    float in_mean, in_norm, out_scale, out_offset; /* the luma plane's u8_in / u8_out maps */
} snn_colour_io;
int snn_model_create7(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                      int prefer_half, int capture_graph, int batch, const snn_colour_io* io, snn_model** out);
/* Video frames around a luma-only model: NV12 (8-bit) or P010-style (2-byte containers) frames at BOTH ends, as a hardware decoder hands them out
 * -- a full-resolution luma plane followed by a half-resolution plane of interleaved CbCr.  Through a struct and an entry point of their own: every
 * earlier struct and entry point keeps its layout and behaviour.  The model is built exactly as snn_model_create5 builds it with SNN_IO_R8 at both
 * ends (SNN_IO_NV12), or as snn_model_create6 builds it with SNN_IO_R16, in_shift = out_shift = shift and out_maxval = maxval (SNN_IO_NV12_16;
 * P010 is maxval 1023, shift 6), so ESPCN still runs as its two fused kernels with the conversions folded in (the fp16 opt-in folds them too).
 * in_mean / in_norm / out_scale / out_offset are the luma plane's maps: limited-range video is mean 16, norm 1/219, scale 219, offset 16 (in
 * units of the bit depth).  The chroma plane [batch][H/2][W/2][2] goes through one more launch, behind the model's on the same stream and inside
 * the recorded graph with capture_graph (it counts towards SNN_GRAPH_MIN_LAUNCHES): snnhip_chroma_up_plan_create with the model's r, maxval, shift
 * and siting (SNN_SITING_LEFT: chroma co-sited with even luma columns, the default of H.264 / HEVC / AV1 streams; SNN_SITING_CENTRE: JPEG /
 * MPEG-1); include/snnhip.h states the arithmetic.  snn_model_describe lists the launch.  Returns -1, before anything is built on the device,
 * for a null struct, a format that is not one of the two, a model that is not one channel in and one channel out at 1..4 times the extent, an odd
 * in_w or in_h, maxval > 4095 (or one that does not fit the container with shift), an unknown siting and batch 0.  The reference has no video
 * frame path (core/inc/snn/color.h only names the layouts). */
enum { SNN_IO_NV12 = 0x201, SNN_IO_NV12_16 = 0x301 }; /* (low byte = the model's channel count) */
enum { SNN_SITING_CENTRE = 0, SNN_SITING_LEFT = 1 };
typedef struct snn_video_io {
    int format; /* SNN_IO_NV12 or SNN_IO_NV12_16, both ends */
    int maxval, shift, siting;
    float in_mean, in_norm, out_scale, out_offset; /* the luma plane's maps */
} snn_video_io;
int snn_model_create8(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                      int prefer_half, int capture_graph, int batch, const snn_video_io* io, snn_model** out);
/* `batch` frames, each H*W luma elements followed by (H/2)*W interleaved chroma elements (bytes for SNN_IO_NV12, 2-byte elements for
 * SNN_IO_NV12_16), into the model's luma frame tensor and its chroma tensor; the download returns `batch` frames of rH*rW + (rH/2)*rW elements.
 * With batch 1 the two planes are copied straight from / to the caller's memory; a larger batch is regrouped through a host buffer (the device
 * tensors stay contiguous [N][H][W][C]).  -1 when the model was not made by snn_model_create8. */
int snn_model_upload_frame_nv12(snn_model* m, const void* frames);
int snn_model_download_frame_nv12(snn_model* m, void* frames);
/* Video in, display out: NV12 / P010 frames at the model's INPUT, packed full-range RGB or RGBA at its output.  Through a struct and an entry point
 * of their own: every earlier struct and entry point keeps its layout and behaviour.  The luma plane's maps follow from `range` and are not given --
 * with k = (maxval + 1) / 256, SNN_RANGE_LIMITED: mean 16k, norm 1 / (219k), scale 219k, offset 16k; SNN_RANGE_FULL: mean 0, norm 1 / maxval, scale
 * maxval, offset 0 -- and the model is built exactly as snn_model_create8 builds it with them, so ESPCN stays two fused kernels with folded ends
 * (the fp16 opt-in folds them too).  One more launch sits behind the model's on the same stream and inside the recorded graph, three launches in
 * all: snnhip_yuv_rgb_plan_create (include/snnhip.h states the arithmetic) takes the model's output luma frame and the ORIGINAL chroma plane
 * [batch][H/2][W/2][2] and writes the RGB frame; the chroma_up launch of snn_model_create8 is not made and no upscaled chroma plane exists.
 * snn_model_upload_frame_nv12 takes the frames; snn_model_download_frame_u8 / _u16 return [batch][rH][rW][C] (C = 3, or 4 with A = maxval << shift);
 * snn_model_download_frame_nv12 returns -1.  snn_model_describe lists the extra launch.  Returns -1, before anything is built on the device, unless
 * the model has one channel in and one channel out at r = 1..4 times the extent, in_w and in_h are even, the formats pair up (SNN_IO_NV12 with
 * SNN_IO_RGB8 / RGBA8, SNN_IO_NV12_16 with SNN_IO_RGB16 / RGBA16), maxval + 1 is a multiple of 256, maxval <= 255 (8-bit) / 4095 (16-bit) and
 * maxval << shift fits the container, siting and range are known, 0 < kr, 0 < kb, kr + kb < 1 and batch >= 1.  The reference has no video frame
 * path (core/inc/snn/color.h only names the layouts; its vendored libyuv converts on the CPU). */
enum { SNN_RANGE_LIMITED = 0, SNN_RANGE_FULL = 1 };
typedef struct snn_video_rgb_io {
    int in_format;  /* SNN_IO_NV12 or SNN_IO_NV12_16 */
    int out_format; /* SNN_IO_RGB8 or SNN_IO_RGBA8; SNN_IO_RGB16 or SNN_IO_RGBA16 for a 16-bit input */
    int maxval, shift, siting, range;
    float kr, kb;
} snn_video_rgb_io;
int snn_model_create9(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                      int prefer_half, int capture_graph, int batch, const snn_video_rgb_io* io, snn_model** out);
/* Capture in, encoder out: RGB8 / RGBA8 frames at the model's INPUT, an NV12 frame (4:2:0, what a hardware encoder takes) at its output.  Through a
 * struct and an entry point of their own: every earlier struct and entry point keeps its layout and behaviour.  The model is built exactly as
 * snn_model_create5 builds it with SNN_IO_R8 at both ends; the luma maps follow from `range` and are not given, as in snn_model_create9 -- in: mean
 * 0, norm 1 / 255 (the full-range luma of snnhip_rgb_luma_plan_create); out: scale 219, offset 16 (SNN_RANGE_LIMITED) or scale 255, offset 0
 * (SNN_RANGE_FULL) -- so ESPCN stays its two fused 8-bit kernels (the fp16 opt-in works too).  Four launches in all, on one stream and all inside
 * the recorded graph with capture_graph: snnhip_rgb_luma_plan_create in front (as snn_model_create7), the two fused kernels, and
 * snnhip_rgb_cbcr_plan_create behind them, from the colour input frame to the chroma plane [batch][rH/2][rW/2][2] (include/snnhip.h states the
 * arithmetic; kr / kb are the matrix of both, BT.601 0.299 / 0.114).  snn_model_upload_frame_u8 takes [batch][H][W][C];
 * snn_model_download_frame_nv12 returns `batch` frames of rH*rW + (rH/2)*rW bytes; snn_model_download_frame_u8 returns -1.  snn_model_describe
 * lists both extra launches.  Returns -1, before anything is built on the device, for a null struct, other formats, a model that is not one channel in
 * and one channel out at r = 2..4 times the extent, an odd r*in_w or r*in_h, an unknown siting or range, a matrix outside 0 < kr, 0 < kb, kr + kb < 1
 * and batch < 1.  16-bit sources (RGB16 -> P010) need a 16-bit luma split that does not exist: not offered. */
typedef struct snn_encode_io {
    int in_format;  /* SNN_IO_RGB8 or SNN_IO_RGBA8 */
    int out_format; /* SNN_IO_NV12 */
    int siting, range;
    float kr, kb;
} snn_encode_io;
int snn_model_create10(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                       int prefer_half, int capture_graph, int batch, const snn_encode_io* io, snn_model** out);
/* NV12 / P010 frames to ANY output size behind a luma-only model: the model runs at its own factor r, then the frame is resampled down to
 * out_w x out_h on the device (720p to 1080p is the x2 model, then 3/4).  Through a struct and an entry point of their own: every earlier struct and
 * entry point keeps its layout and behaviour.  `video` is snn_model_create8's struct and the model is built exactly as snn_model_create8 builds it,
 * so ESPCN stays its two fused kernels with folded ends (the fp16 opt-in works too).  Two launches sit behind the model's on the same stream and
 * inside the recorded graph with capture_graph (they count towards SNN_GRAPH_MIN_LAUNCHES), four in all: snnhip_plane_fit_plan_create with C = 1
 * from the model's output luma frame rH x rW to out_h x out_w, and with C = 2 from the ORIGINAL chroma plane H/2 x W/2 to out_h/2 x out_w/2 with
 * the stream's siting (include/snnhip.h states the arithmetic).  There is no chroma_up launch and no r-fold chroma plane.
 * snn_model_upload_frame_nv12 is unchanged; snn_model_download_frame_nv12 returns `batch` frames of out_h*out_w + (out_h/2)*out_w elements;
 * snn_model_describe lists both launches.  Returns -1, before anything is built on the device, for a null struct, for what snn_model_create8
 * refuses, for an out_w or out_h that is odd or below 2 and for out_w / in_w or out_h / in_h outside [1/2, 4]; and, once the model file gives r,
 * for an output larger than r * in or smaller than r * in / 2 on either axis (the logged message names r and says which r would fit).
 * RGB output at a fitted size and fitted RGB8 colour frames are snn_model_create13 below.  Not offered: grey frames (the plan itself takes them:
 * snnhip_plane_fit_plan_create), ratios below 1/2.  The reference has nothing for this: its vendored libyuv scales planes on the CPU with box / bilinear filters. */
typedef struct snn_fit_io {
    snn_video_io video;
    int out_w, out_h;
} snn_fit_io;
int snn_model_create11(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                       int prefer_half, int capture_graph, int batch, const snn_fit_io* io, snn_model** out);
/* Planar 4:2:0 frames (I420 / I010: ffmpeg's yuv420p / yuv420p10le, what dav1d, libvpx and libavcodec decode to and x264, x265 and SVT-AV1 take)
 * around a luma-only model, and plane pointers with row pitches for every video end.  Through a struct and an entry point of their own: every
 * earlier struct and entry point keeps its layout and behaviour.  Four paths, each built exactly as its NV12 counterpart -- the two fused ESPCN
 * kernels with folded ends (the fp16 opt-in works too), every launch on one stream and inside the recorded graph with capture_graph -- and with the
 * same number of launches; no launch interleaves or splits chroma anywhere:
 *     planar -> the same planar format, r-fold     3 launches   snn_model_create8's path: snnhip_chroma_up_plan_create, C = 1 over 2 * batch planes
 *     planar -> planar at out_w x out_h            4 launches   snn_model_create11's path and rules: two snnhip_plane_fit_plan_create, chroma C = 1
 *     planar -> RGB8 / RGBA8 (RGB16 / RGBA16)      3 launches   snn_model_create9's path: snnhip_yuv_rgb_planar_plan_create
 *     RGB8 / RGBA8 -> SNN_IO_I420                  4 launches   snn_model_create10's path: snnhip_rgb_luma in front, snnhip_rgb_cbcr_planar_plan_create behind
 * The device chroma tensors are [2 * batch][h][w][1]: plane 2n is Cb, 2n + 1 Cr of frame n (include/snnhip.h).  The luma plane's maps follow from
 * `range` on every path, as snn_model_create9 / snn_model_create10 state them; kr / kb are the matrix of the RGB end (not looked at planar to planar).
 * snn_model_describe lists the extra launches.  Returns -1, before anything is built on the device, for a null struct, formats that do not pair up
 * as above, a fitted size together with an RGB end, and everything the NV12 counterpart of the path refuses: a model that is not one channel in and
 * out, odd extents, maxval other than 255 (8-bit) or outside 255 .. 4095 (16-bit) or with maxval + 1 not a multiple of 256, a shift that does not fit, an unknown
 * siting or range, a matrix outside 0 < kr, 0 < kb, kr + kb < 1, batch < 1; the fitted size's rules (even, ratio in [1/2, 4]); and, once the model file
 * gives r, r = 1 with RGB in and a fitted size outside [r * in / 2, r * in].  RGB output at a fitted size comes through snn_model_create13 below,
 * not through this struct.  Not offered: 4:2:2 / 4:4:4 and packed layouts, BGR order, 16-bit RGB -> I010, pitched DEVICE surfaces (the device tensors
 * stay dense). */
enum { SNN_IO_I420 = 0x401, SNN_IO_I420_16 = 0x501 }; /* (low byte = the model's channel count) */
typedef struct snn_planar_io {
    int in_format;  /* SNN_IO_I420, SNN_IO_I420_16, or SNN_IO_RGB8 / SNN_IO_RGBA8 (capture in) */
    int out_format; /* planar in: the same planar format, or RGB8 / RGBA8 (8-bit), RGB16 / RGBA16 (16-bit); RGB in: SNN_IO_I420 */
    int maxval, shift, siting, range;
    float kr, kb;
    int out_w, out_h; /* 0, 0: r times the input; otherwise the fitted size, planar in and planar out only */
} snn_planar_io;      /* 10 * 4 bytes */
int snn_model_create12(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                       int prefer_half, int capture_graph, int batch, const snn_planar_io* io, snn_model** out);
/* RGB frames at ANY output size behind a luma-only model: what a display path asks for (720p to 1080p through the x2 or the x3 model, 1080p to
 * 1440p).  Through a struct and an entry point of their own: every earlier struct and entry point keeps its layout, behaviour and refusals
 * (snn_model_create12 still refuses a fitted size together with an RGB end).  Two paths, every launch on one stream and inside the recorded graph
 * with capture_graph:
 *     NV12 / P010 / I420 / I010 -> RGB(A) at out_w x out_h    4 launches   the model built exactly as snn_model_create9 builds it (planar planes:
 *                                                                          snn_model_create12's RGB path), then [luma fit] and [rgb fit]
 *     RGB8 / RGBA8 -> the same format at out_w x out_h        5 launches   the model built exactly as snn_model_create7 builds it with the luma maps
 *                                                                          in_mean 0, in_norm 1 / 255, out_scale 255, out_offset 0: snnhip_rgb_luma in
 *                                                                          front, then [luma fit] and [rgb fit]
 * [luma fit] is snnhip_plane_fit_plan_create with C = 1 (centre) from the model's r-fold luma frame to out_h x out_w, exactly as in
 * snn_model_create11's path; [rgb fit] is snnhip_rgb_fit_plan_create from that plane and the ORIGINAL chroma planes (or the colour frame that went
 * in) to the RGB frame (include/snnhip.h states the arithmetic).  No r-fold chroma plane and no r-fold RGB frame exists anywhere; ESPCN stays its
 * two fused kernels with folded ends (the fp16 opt-in works too).  snn_model_upload_frame_nv12 / _planes / _u8 take the frames as on the paths
 * above; snn_model_download_frame_u8 / _u16 return [batch][out_h][out_w][C] (A = maxval << shift from video, the alpha of the source pixel
 * underneath from RGBA8); snn_model_describe lists both launches; snn_model_reference_frame / snn_model_frame_metrics work on the fitted frame (one
 * packed plan).  out_w and out_h need not be even.  Returns -1, before anything is built on the device, for a null struct, for what
 * snn_model_create9 / snn_model_create12 (video in) or snn_model_create7 (RGB in) refuses, for formats that do not pair up (video in: RGB8 / RGBA8
 * for 8-bit, RGB16 / RGBA16 for 16-bit; RGB in: the same format out), for out_w or out_h below 1 and for out / in outside [1/2, 4] (video in) or
 * [1, 4] (RGB in) on either axis; and, once the model file gives r, for an output outside [r * in / 2, r * in] on either axis or, with RGB in, below
 * the input's extent -- the colour frame is never shrunk, so r = 1 then permits out = in alone (the logged message names r and says which r would
 * fit).  Not offered: grey frames at a fitted size (the plan itself takes them: snnhip_plane_fit_plan_create), ratios below 1/2, RGB16 sources, BGR
 * order, 4:2:2 / 4:4:4, a fused luma-fit + RGB launch. */
typedef struct snn_rgb_fit_io {
    int in_format;  /* SNN_IO_NV12, SNN_IO_NV12_16, SNN_IO_I420, SNN_IO_I420_16, or SNN_IO_RGB8 / SNN_IO_RGBA8 */
    int out_format; /* video in: RGB8 / RGBA8 (8-bit), RGB16 / RGBA16 (16-bit); RGB in: the same format */
    int maxval, shift, siting, range; /* video in: as snn_video_rgb_io; RGB in: not looked at */
    float kr, kb;
    int out_w, out_h; /* the size of the RGB frame that comes back; need not be even */
} snn_rgb_fit_io;     /* 10 * 4 bytes */
int snn_model_create13(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                       int prefer_half, int capture_graph, int batch, const snn_rgb_fit_io* io, snn_model** out);
/* Video frames in front of an RGB(A) model: a decoder's NV12 / P010 / I420 / I010 frame of ANY even size goes straight to the model's normalised input
 * tensor -- ResNet-18, MobileNetV2, YOLOv3-tiny, Candy -- in ONE launch in front of the model's own (include/snnhip.h, snnhip_yuv_tensor_plan_create,
 * states the arithmetic: yuv_rgb's unrounded RGB value per source pixel, resize's sampling rule, (sample - mean) * norm).  Through a struct and an
 * entry point of their own: every earlier struct and entry point keeps its layout, behaviour and refusals.  Here in_w, in_h and in_c are the MODEL's
 * input extent and channels, in_c = 3 (R, G, B) or 4 (+ alpha); src_w x src_h is the frame's.  The model is built exactly as snn_model_create4 builds
 * it, or, with an 8-bit out_format, as snn_model_create5 builds it with in_format = SNN_IO_FLOAT and that out_format, out_scale and out_offset (Candy:
 * video in, RGB8 out).  The launch, "[yuv tensor]" in snn_model_describe, runs on the model's stream from the frame's device planes into the model's
 * own input tensor, sits inside the recorded graph with capture_graph and counts towards SNN_GRAPH_MIN_LAUNCHES; prefer_half models get its fp16
 * instance.  The plane tensors and the input tensor are allocated once: a recorded graph replays across uploads.  snn_model_upload_frame_nv12 takes
 * dense frames (src_h * src_w luma elements, then (src_h / 2) * src_w interleaved chroma elements), snn_model_upload_frame_planes pitched planes
 * (n_planes = 2, or 3 for the planar formats); snn_model_upload_input and snn_model_upload_input_u8 return -1 on such a model;
 * snn_model_download_input returns the tensor the launch wrote; the downloads are the model's usual ones.  Returns -1, before anything is built on
 * the device, for a null struct, an in_format that is none of the four, an out_format that is neither SNN_IO_FLOAT nor an 8-bit format, in_c outside
 * {3, 4}, an odd or non-positive src_w / src_h, in_w or in_h below 1, batch below 1, an unknown filter, siting or range, kr / kb outside 0 < kr,
 * 0 < kb, kr + kb < 1, maxval + 1 not a multiple of 256, maxval above 255 (8-bit) / 4095 (16-bit) and a maxval << shift that does not fit the
 * container.  Not offered: anti-aliased shrinking (the sampler is the reference's plain bilinear resize), letterboxing and crop rectangles,
 * 4:2:2 / 4:4:4, BGR order, and video in front of the luma-only model paths, which have their own entry points above. */
enum { SNN_FILTER_NEAREST = 0, SNN_FILTER_LINEAR = 1 };
typedef struct snn_video_tensor_io {
    int in_format;    /* SNN_IO_NV12, SNN_IO_NV12_16, SNN_IO_I420 or SNN_IO_I420_16 */
    int out_format;   /* SNN_IO_FLOAT, or an 8-bit format of the model output's own channel count */
    int src_w, src_h; /* the frame's luma extent, both even */
    int maxval, shift, siting, range; /* as snn_video_rgb_io */
    float kr, kb;
    int filter;       /* SNN_FILTER_NEAREST or SNN_FILTER_LINEAR */
    float means[4], norms[4]; /* t = (sample - means[c]) * norms[c]; three are used */
    float alpha;      /* channel 3 of a 4-channel input */
    float out_scale[4], out_offset[4]; /* an 8-bit out_format: as snn_frame_io */
} snn_video_tensor_io; /* 28 * 4 bytes */
int snn_model_create14(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                       int prefer_half, int capture_graph, int batch, const snn_video_tensor_io* io, snn_model** out);
/* Encoder frames behind an RGB(A) model: the model's output tensor leaves as the planes of a 4:2:0 frame of the same extent -- NV12 / P010 / I420 /
 * I010, what a hardware or software encoder takes -- in ONE launch behind the model's last stage (include/snnhip.h, snnhip_tensor_yuv_plan_create,
 * states the arithmetic: p = clamp(x * out_scale + out_offset, 0, maxval), the luma code, the chroma differences decimated 2 x 2, the chroma codes).
 * With snn_model_create14's frame in front, "decoder -> RGB model -> encoder" runs with no float frame and no RGB frame crossing the host link.
 * Through a struct and an entry point of their own: every earlier struct and entry point keeps its layout, behaviour and refusals.  The model is
 * built exactly as snn_model_create4 builds it; with an 8-bit in_format exactly as snn_model_create5 builds it with that in_format, in_means, in_norms
 * and a float output; with a video in_format exactly as snn_model_create14 builds it from video_in with a float output.  The launch, "[tensor yuv]"
 * in snn_model_describe, runs on the model's stream from the model's own output tensor (the fp16 tensor of a prefer_half model) into plane tensors
 * that are allocated once, sits inside the recorded graph with capture_graph and counts towards SNN_GRAPH_MIN_LAUNCHES.  snn_model_download_frame_nv12
 * returns dense frames (H * W luma elements, then (H / 2) * W interleaved chroma elements; SNN_IO_NV12 / _NV12_16), snn_model_download_frame_planes
 * pitched planes (n_planes = 2, or 3 for the planar formats); snn_model_reference_frame* and snn_model_frame_metrics work on them as for the other
 * video ends (one luma row and two chroma rows per image); snn_model_download_output, snn_model_download_frame_u8 and _u16 return -1 on such a
 * model.  Returns -1, before anything is built on the device, for a null struct, an out_format that is none of the four, an in_format that is
 * neither SNN_IO_FLOAT, an 8-bit format of in_c channels nor one of the four video formats, a video in_format that video_in.in_format does not
 * repeat or whose video_in.out_format is not SNN_IO_FLOAT, everything snn_model_create14 refuses about video_in, batch below 1, an unknown siting or
 * range, kr / kb outside 0 < kr, 0 < kb, kr + kb < 1, maxval + 1 not a multiple of 256, maxval above 255 (8-bit) / 4095 (16-bit) and a
 * maxval << shift that does not fit the container; and, once the model file gives the output, for a model whose output has not 3 or 4 channels or an
 * odd extent.  Not offered: resizing at this end (a fitted encoder size would be plane_fit behind it), 4:2:2 / 4:4:4, BGR order, a cubic or longer
 * decimation filter, and folding the conversion into the model's last convolution. */
typedef struct snn_tensor_video_io {
    int in_format;   /* SNN_IO_FLOAT; an 8-bit frame format of the model input's channel count (in_means / in_norms as snn_frame_io);
                        or SNN_IO_NV12 / _NV12_16 / _I420 / _I420_16: then video_in describes the frame in front, exactly as snn_model_create14 takes it */
    int out_format;  /* SNN_IO_NV12, SNN_IO_NV12_16, SNN_IO_I420 or SNN_IO_I420_16 */
    int maxval, shift, siting, range; /* the OUTPUT stream's, as snn_video_rgb_io */
    float kr, kb;
    float out_scale[4], out_offset[4]; /* three are used: p = clamp(x * out_scale[c] + out_offset[c], 0, maxval), full-range RGB at the output depth */
    float in_means[4], in_norms[4];    /* an 8-bit in_format: as snn_frame_io */
    snn_video_tensor_io video_in;      /* looked at only with a video in_format; its out_format must be SNN_IO_FLOAT */
} snn_tensor_video_io; /* 52 * 4 bytes */
int snn_model_create15(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                       int prefer_half, int capture_graph, int batch, const snn_tensor_video_io* io, snn_model** out);
int snn_model_download_input(snn_model* m, float* nhwc); /* the model's input tensor, [batch x] H x W x C floats (what [yuv tensor] wrote, or the last upload) */
/* Frames as plane pointers with row pitches (ffmpeg's data[] / linesize[]).  `planes` holds batch * n_planes pointers, frame by frame, in the order
 * Y, Cb, Cr (a YV12 caller swaps the last two) for a planar end, n_planes = 3; Y, CbCr for the NV12 / P010 ends of models made by snn_model_create8
 * / 9 / 10 / 11, n_planes = 2 (pitched NV12 surfaces).  pitch_bytes[n_planes] is the row pitch of each plane, the same for every frame.  Planes that
 * are tight (pitch = the row's bytes) and adjacent in memory in the device tensor's order are copied straight; anything else is gathered through the
 * model's host staging buffer row by row with memcpy: padding bytes are never read, and a download writes width * element size bytes per row and
 * leaves the padding untouched.  -1 for a null argument (a null plane pointer among them), an n_planes that does not match that end of the model, a
 * pitch below the row's bytes, or an RGB end.  snn_model_upload_frame_nv12 / _download_frame_nv12 keep their behaviour and return -1 on planar ends. */
int snn_model_upload_frame_planes(snn_model* m, const void* const* planes, const int* pitch_bytes, int n_planes);
int snn_model_download_frame_planes(snn_model* m, void* const* planes, const int* pitch_bytes, int n_planes);
/* Frame quality on the device: PSNR and SSIM of the model's output frame against a ground-truth frame, without downloading the output
 * (include/snnhip.h, snnhip_frame_metrics_plan_create, states the definition).  They sit on an existing model: no entry point of its own.
 * snn_model_reference_frame takes the ground-truth frame in exactly the dense layout this model's download function takes
 * (snn_model_download_frame_u8 / _u16 / _nv12); snn_model_reference_frame_planes has the arguments and the acceptance rules of
 * snn_model_download_frame_planes.  The first call to either allocates device-resident reference tensors and one metrics plan per output plane
 * tensor: a packed R8 / RGB8 / RGBA8 or 16-bit frame one plan with C = 1, 3 or 4; NV12 / P010 a luma plan (C = 1) and a CbCr plan (C = 2); I420 /
 * I010 a luma plan and one C = 1 plan over the 2 * batch chroma planes; a fitted out_size the fitted planes.  A later call replaces the reference.
 * Both return -1, with a logged message, on a model whose output is a float tensor (and for a null argument).
 * snn_model_frame_metrics runs the plans on the output of the last run against the reference, on the model's stream behind that run and outside the
 * recorded graph (a replayed graph is not changed: snn_model_run launches what it launched before), waits, and writes one row per (image, plane,
 * channel), image-major: the frame's channels (plane 0), then on a video output the chroma plane's -- plane 1 with channels 0 (Cb) and 1 (Cr) for
 * NV12 / P010, planes 1 (Cb) and 2 (Cr) with channel 0 for I420 / I010.  psnr_db is +inf for equal planes; ssim is 1.0 exactly for them.  Returns
 * the row count, or -1 with a logged message when no reference was set, for a null argument and for max_rows below the count. */
typedef struct snn_frame_metrics {
    int image, plane, channel;
    unsigned long long sse, pixels;
    double psnr_db, ssim;
} snn_frame_metrics;
int snn_model_reference_frame(snn_model* m, const void* frame);
int snn_model_reference_frame_planes(snn_model* m, const void* const* planes, const int* pitch_bytes, int n_planes);
int snn_model_frame_metrics(snn_model* m, snn_frame_metrics* rows, int max_rows);
int snn_model_batch(snn_model* m);
/* the C-ABI handles behind a model: its context (device + stream) and the device tensor of its last stage's output (borrowed) */
struct snnhip_ctx* snn_model_hip_ctx(snn_model* m);
struct snnhip_tensor* snn_model_output_tensor(snn_model* m);
int snn_model_destroy(snn_model* m);
int snn_model_upload_input(snn_model* m, const float* nhwc);      /* [batch x] H x W x C floats */
int snn_model_run(snn_model* m);                                   /* MixedInferenceCore::run (enqueue + one sync) */
/* RunParameters::deferSync: enqueue the inference and return; several inferences stay in flight on the model's stream until
 * snn_model_sync (throughput mode; the reference waits once per inference, core.cpp:203) */
int snn_model_run_async(snn_model* m);
int snn_model_sync(snn_model* m);
int snn_model_output_dims(snn_model* m, int hwc[3]);
int snn_model_download_output(snn_model* m, float* nhwc);
/* SNNModelOutput of the next runs (snn.h ModelType: 0 CLASSIFICATION, 1 DETECTION, 2 SEGMENTATION, 3 OTHER; MixedInferenceCore::run, core.cpp:228-237) */
int snn_model_set_type(snn_model* m, int model_type);
int snn_model_classifier_output(snn_model* m);                             /* 1-based arg-max of the last stage, 0 = none */
int snn_model_detections(snn_model* m, float* rows6, int max_rows);         /* YOLO stage output {class, score, x, y, w, h}; returns the row count */
/* Input pre-processing on the device, the demo's call sequence (modelInference.cpp:92-97): decoded 8-bit image (1 / 3 / 4 channels) ->
 * convertToRGBA32FAndNormalize(means, norms) -> resize to the model's input size with (resize_means, resize_norms), bilinear.
 * The model must take a 4-channel input (RGBA texture). */
int snn_model_upload_input_u8(snn_model* m, const unsigned char* pixels, int w, int h, int channels, const float means[4], const float norms[4],
                              const float resize_means[4], const float resize_norms[4]);
int snn_model_num_stages(snn_model* m);
/* *fused_away: bit 0 = the stage's work moved into a later stage's fused plan; bit 1 = the stage is issued on the side stream beside the
 * previous launching stage (SNN_BRANCH_OVERLAP=1) */
int snn_model_stage_info(snn_model* m, int stage, char* name, int name_len, int hwc[3], int* fused_away);
int snn_model_download_stage(snn_model* m, int stage, float* nhwc);
int snn_model_describe(snn_model* m, char* buf, int buflen);
/* The plan a stage launches after fusion (0 steps: input layer, CPU stage, or folded into a later stage's fused plan): kernel description and
 * algorithmic cost of each of its launches, per-launch HIP-event profiling (snnhip_plan_profile_*) and the summed cost of one inference. */
int snn_model_stage_plan_steps(snn_model* m, int stage);
int snn_model_stage_plan_step(snn_model* m, int stage, int step, char* desc, int desc_len, double* flops, double* bytes);
int snn_model_profile_enable(snn_model* m, int enable);
int snn_model_profile_read(snn_model* m, int stage, int step, double* total_ms, int* launches);
/* run launch by launch instead of replaying the recorded hipGraph (1) / replay again (0): what a launch trace (snnhip_trace_begin) needs --
 * a replayed graph never calls the plans */
int snn_model_suspend_replay(snn_model* m, int suspend);
int snn_model_cost(snn_model* m, double* flops, double* bytes);
/* per-stage device timers of the last run, milliseconds (MixedInferenceCore::writeTimeStat); returns count written */
int snn_model_time_stats(snn_model* m, char* names, int names_len, double* ms, int max_entries);

/* ---- multi-device pool (shadernn_amd/host/pool.cpp; SURVEY 8b "Threading" + 8e): one replica = one host thread + HipContext + stream per entry of
 * devices[] (an entry may repeat), each owning one MixedInferenceCore per micro-batch slot of its share [g*B/G, (g+1)*B/G) of the global batch.
 * Weights are loaded per replica, nothing crosses devices on the data path.  micro_batch 0 = a replica's share in one pass.
 * The reference is single-device (vulkanBackend.cpp:30-31); its benchmark loop (inferenceProcessor.cpp:84-86) is what one replica runs. */
typedef struct snn_pool snn_pool;
int snn_pool_create(const char* json_path, const int* devices, int n_devices, int in_w, int in_h, int in_c, int prefer_half, int capture_graph,
                    int global_batch, int micro_batch, snn_pool** out);
int snn_pool_destroy(snn_pool* p);
int snn_pool_replicas(snn_pool* p);
int snn_pool_shard(snn_pool* p, int replica, int* first_image, int* images, int* slots);
int snn_pool_output_dims(snn_pool* p, int hwc[3]);
int snn_pool_upload_input(snn_pool* p, const float* nhwc);              /* global_batch x H x W x C floats; every replica takes its images */
/* all replicas released together; each enqueues `steps` passes over its slots (deferSync) and waits once; returns when the slowest is done
 * (seconds = that wall time: the in-process form of bench.py's barrier + MAX over ranks) */
int snn_pool_run(snn_pool* p, int steps, double* seconds);
int snn_pool_download_output(snn_pool* p, float* nhwc);                 /* gather through host memory: global_batch x outH x outW x outC floats */
/* the edge collective of SURVEY 8e: one ncclAllGather per slot over the replicas' streams (librccl.so loaded at run time), rank 0's copy handed to
 * the host.  -3: the replicas do not have equal shares or two of them share a device (RCCL needs one rank per device); -4: RCCL unavailable / failed */
int snn_pool_allgather_output_rccl(snn_pool* p, float* nhwc_rank0);

/* Restatement of ShaderUnitTest::snnConvTestWithLayer (shaderUnitTest.cpp:174-280): input HWC floats, weights as OC*IC
 * matrices of k x k (flat OIHW), bias[OC], optional BN (4 arrays of OC or NULL), pad: 0 constant 1 replicate 2 reflect.
 * Writes the layer dump and returns its path in dump_path; the dump is the reference's ".dump" format. */
int snn_conv_test_with_layer(int device, const float* input_hwc, const float* weights_oihw, const float* bias, int width, int height, int in_channels,
                             int out_channels, int kernel, int stride, int pad, int use_bn, const float* bn_gamma, const float* bn_mean,
                             const float* bn_var, const float* bn_beta, char* dump_path, int dump_path_len);

/* Host-only (no GPU): parse the JSON model, build the layer DAG and the inference graph for a W x H x C input and print one
 * line per layer: "<index>|<name>|<exec type>|<out W>x<out H>x<out C>|<inputs>".  Exercises ModelParser, layerFactory,
 * topological sort and the shape rules exactly as MixedInferenceCore::create would. */
int snn_graph_summary(const char* json_path, int in_w, int in_h, int in_c, char* buf, int buflen);

/* Host-only: YOLOLayer's decode + NMS (yololayer.cpp:114-226) on two NHWC heads of net/32 and net/16 cells x 18 channels */
int snn_yolo_decode(const float* head_coarse, const float* head_fine, int net_size, float* rows6, int max_rows);

/* Host-only: parse `text` as ONE JSON number with the model loader's own parser (ic2/json.h); returns 0 and the value, -1 if it is not a number.
 * Test hook for the loader's number grammar (overflow saturates to +-HUGE_VAL, underflow gives +-0 / a denormal, like the reference's strtod). */
int snn_json_number(const char* text, double* out);

/* Host-only: what snn_model_create<entry> (entry = 5..15, `io` that entry point's struct or NULL) resolves its struct to for an in_w x in_h x in_c
 * input and `batch` images, before any model file is opened: -1 where the entry point refuses the request, otherwise 0 and one canonical text line in
 * buf, "<the model's own end formats and maps> | <the frames the caller uploads and gets back, and their parameters> | entry=<name>".  Test hook for
 * the "built exactly as" statements above: two requests that name the same model resolve to the same first part (shadernn_amd/host/snn/frames.h). */
int snn_frames_resolve(int entry, const void* io, int in_w, int in_h, int in_c, int batch, char* buf, int buflen);

/* ".dump" reader (image.cpp:300-311): returns W,H,D,C and, if out != NULL, the RGBA32F pixels ([D][H][W][4] floats). */
int snn_dump_read(const char* path, int whdc[4], float* out, long out_floats);

#ifdef __cplusplus
}
#endif
#endif
