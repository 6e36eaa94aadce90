/*
 * snnhip.h -- thin C-ABI between ShaderNN's C++ host side and the MI355X (gfx950) HIP operator kernels.
 *
 * This is the drop-in boundary: plain pointers and sizes only, no C++ or
 * torch types.  Everything the reference's per-layer "render pass" does on the GPU is reachable through these
 * entry points:
 *
 *   reference interface being replaced                                   | entry point here
 *   ---------------------------------------------------------------------+------------------------------------------
 *   createDefaultContext / VulkanBackend ctor                            | snnhip_ctx_create / _create_on_stream
 *     core/src/contextFactory.cpp:21-32, core/src/ic2/vulkanBackend.cpp:28-41
 *   ImageTextureVulkan::resetTexture / upload / download / attach        | snnhip_tensor_alloc / _upload* / _download* / _wrap
 *     core/src/imageTextureVulkan.cpp:188-243, core/inc/snn/imageTexture.h:69-147,301-313
 *   Conv2DLayerVulkan::createCS + VulkanRenderPass ctor (weights, spec    | snnhip_conv2d_plan_create
 *     constants, pipeline)  core/src/ic2/conv2dVulkan.cpp:38-239, vulkanRenderpass.cpp:103-178
 *   SeparableConv2DLayerVulkan::createCS                                 | snnhip_depthwise_plan_create
 *     core/src/ic2/separableconvolutionVulkan.cpp:32-160
 *   DenseLayerVulkan::createCS / DenseLayer::computeImageTexture         | snnhip_dense_plan_create
 *     core/src/ic2/denselayerVulkan.cpp:33-126, denselayer.cpp:27-38
 *   SubpixelLayerVulkan::createCS                                        | snnhip_subpixel_plan_create
 *     core/src/ic2/subpixelmergeVulkan.cpp:29-91
 *   Add/Activation/BatchNorm/Pooling/Pad/Upsample/InstanceNorm/Concat    | snnhip_eltwise_plan_create ... (section "next ops")
 *   VulkanRenderPass::run (bind + Dispatch + barrier)                    | snnhip_plan_run
 *     core/src/ic2/vulkanRenderpass.cpp:181-260
 *   VulkanBackend::sync (QueueSubmitAndWait)                             | snnhip_sync
 *     core/src/ic2/vulkanBackend.cpp:97-106
 *   DeviceTimer (timestamp query pool)  core/inc/snn/deviceTimer.h:20-51 | snnhip_timer_*
 *
 * Conventions: every function returns 0 (SNNHIP_OK) or a negative SNNHIP_E_* code; snnhip_last_error() gives a
 * thread-local human-readable message.  The C++ wrapper turns non-zero into SNN_RIP to keep the reference's
 * abort-on-error behaviour (core/inc/snn/utils.h:57-62).  Tensors are plain NHWC fp32 buffers in HBM (the
 * reference's RGBA "C4HW4" 3-D textures exist only at the API edge: *_c4hw4 upload/download convert).
 * All work is enqueued on the context's HIP stream; nothing synchronises except snnhip_sync, the download
 * functions and snnhip_timer_elapsed_ms.
 */
#ifndef SNNHIP_H
#define SNNHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNNHIP_OK 0
#define SNNHIP_E_INVALID (-1)     /* bad argument / shape mismatch                          */
#define SNNHIP_E_HIP (-2)         /* a HIP runtime call failed (message has the hipError)   */
#define SNNHIP_E_UNSUPPORTED (-3) /* valid request that no kernel variant implements        */
#define SNNHIP_E_NOMEM (-4)
#define SNNHIP_E_GUARD (-5)       /* SNNHIP_GUARD=1: a kernel wrote outside one of the library's device allocations */

typedef struct snnhip_ctx snnhip_ctx;
typedef struct snnhip_tensor snnhip_tensor;
typedef struct snnhip_plan snnhip_plan;
typedef struct snnhip_timer snnhip_timer;

/* activation ids: specialisation constant 15 of the conv shaders (conv2dVulkan.cpp:58-72) */
enum {
    SNNHIP_ACT_NONE = 0,
    SNNHIP_ACT_RELU = 1,
    SNNHIP_ACT_RELU6 = 2,
    SNNHIP_ACT_TANH = 3,
    SNNHIP_ACT_SIGMOID = 4,
    SNNHIP_ACT_LEAKY = 5,
    SNNHIP_ACT_SILU = 6,       /* x*sigmoid(x) */
    SNNHIP_ACT_SILU_QUIRK = 7  /* bit-for-bit model of the reference SiLU bug (vk_conv2d.comp:336-339) */
};
/* padding mode: specialisation constant 16 (conv2dVulkan.cpp:74-81) */
enum { SNNHIP_PAD_NONE = 0, SNNHIP_PAD_CONSTANT = 1, SNNHIP_PAD_REPLICATE = 2, SNNHIP_PAD_REFLECT = 3 };
/* element types.  SNNHIP_F16 = IEEE half storage (the reference's RGBA16F textures / "preferHp", inferencegraph.h ColorFormat::RGBA16F):
 * tensors hold halfs in HBM, kernels convert on load, accumulate in fp32 (fp16-input MFMA for the convolutions) and round to nearest even
 * on store.  The host-side upload / download entry points always speak fp32 and convert. */
enum { SNNHIP_F32 = 0, SNNHIP_F16 = 1, SNNHIP_U8 = 2 /* 8-bit frames: input of snnhip_image_u8_plan_create / snnhip_u8_in_plan_create, output of
                                                          snnhip_u8_out_plan_create, and the two ends of a chain that starts / ends with those plans */,
       SNNHIP_U16 = 3 /* 16-bit frames (10 / 12 / 16-bit video in 2-byte containers): input of snnhip_u16_in_plan_create, output of
                         snnhip_u16_out_plan_create, and the two ends of a chain that starts / ends with those plans */ };

/* ---- context -------------------------------------------------------------------------------------- */

typedef struct {
    char name[128];
    int compute_units;
    int lds_bytes_per_cu;
    size_t hbm_bytes;
    int device;
} snnhip_device_info;

int snnhip_ctx_create(int device, snnhip_ctx** out);
/* Uses a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) instead of creating one. */
int snnhip_ctx_create_on_stream(int device, void* hip_stream, snnhip_ctx** out);
int snnhip_ctx_destroy(snnhip_ctx* ctx);
int snnhip_ctx_info(snnhip_ctx* ctx, snnhip_device_info* info);
void* snnhip_ctx_stream(snnhip_ctx* ctx);
/* Two independent operators side by side (MI355X-side design; the reference records one command buffer on one queue,
 * vulkanBackend.cpp:80-95).  snnhip_ctx_fork: the context's SIDE stream (created on first use) waits for everything enqueued on the main stream
 * so far, and every plan run on this context goes to the side stream until snnhip_ctx_main switches back (the side work keeps running);
 * snnhip_ctx_join makes the main stream wait for the side stream's work.  Valid inside a graph capture (the side stream joins the
 * capture through the fork event and must be joined before the capture ends).  Used by the host mirror for residual-block pairs such as
 * ResNet's 3x3 stride-2 convolution and the 1x1 stride-2 downsample that read the same tensor. */
int snnhip_ctx_fork(snnhip_ctx* ctx);
int snnhip_ctx_main(snnhip_ctx* ctx);
int snnhip_ctx_join(snnhip_ctx* ctx);
/* Launch groups (HIP extension, round 6): plans that report snnhip_plan_groupable (today: the K-split convolutions of conv2d_ksplit.hip) and are run
 * between _group_begin and _group_end are launched by _group_end -- two independent ones that fit one grid as ONE kernel launch (a ResNet stage entry's
 * 3x3 stride-2 convolution and the 1x1 stride-2 downsample beside it: the short blocks of the second fill the CUs the first leaves idle), anything
 * else one by one.  The caller guarantees that the grouped plans do not consume each other's outputs; every other plan run inside a group is launched
 * at once, as usual.  Valid inside a graph capture. */
int snnhip_ctx_group_begin(snnhip_ctx* ctx);
int snnhip_ctx_group_end(snnhip_ctx* ctx);
int snnhip_plan_groupable(const snnhip_plan* plan);
int snnhip_sync(snnhip_ctx* ctx);
const char* snnhip_last_error(void);
const char* snnhip_version(void);
/* Options: the kernel-selection / fusion switches of DESIGN.md section 8 (names "SNNHIP_..."), process-wide.  A value set here wins over the
 * environment variable of the same name (the fallback, read when a plan is created); value == NULL removes the override.  The reference has no
 * counterpart: its shader variants are picked by MixedInferenceCore's options struct (core/inc/snn/core.h: dumpOutputs, mrtMode, weightMode ...). */
int snnhip_set_option(const char* name, const char* value);
const char* snnhip_get_option(const char* name); /* the effective value (override, else environment), or NULL */
/* Device-side guard mode (SURVEY section 5's "compute-sanitizer equivalent"; the reference has none, core/CMakeLists.txt:235).  With SNNHIP_GUARD=1 in the
 * environment when the library makes its first allocation, every device allocation of the library -- tensors, packed weights, split-K / statistics
 * scratch -- sits between two 64 KiB red zones filled with 0xFF bytes (a NaN in fp32 and in fp16: an out-of-bounds READ that reaches a result
 * poisons it, and fresh tensors / scratch are poisoned the same way, so a read of something never written shows too), the tensor flush against the
 * zone behind it.  snnhip_sync (and snnhip_guard_check) then verifies every red zone of the context's device and returns SNNHIP_E_GUARD naming
 * the allocation a kernel wrote outside of.  snnhip_guard_selftest writes one byte `offset` bytes past the END of a tensor (offset < 0: in front
 * of it) from a kernel -- the deliberate fault the checker's own test uses.  tools/sanitize.sh runs the fuzz and bench-size tests under it. */
int snnhip_guard_active(void);
int snnhip_guard_check(snnhip_ctx* ctx);
int snnhip_guard_selftest(snnhip_ctx* ctx, snnhip_tensor* t, long offset);

/* ---- tensors: NHWC fp32 in HBM ------------------------------------------------------------------- */

int snnhip_tensor_alloc(snnhip_ctx* ctx, int n, int h, int w, int c, int dtype, snnhip_tensor** out);
/* Borrow device memory owned by someone else (a torch tensor, another tensor's storage). Never freed here. */
int snnhip_tensor_wrap(snnhip_ctx* ctx, void* device_ptr, int n, int h, int w, int c, int dtype, snnhip_tensor** out);
int snnhip_tensor_free(snnhip_tensor* t);
int snnhip_tensor_dims(const snnhip_tensor* t, int dims_nhwc[4]);
void* snnhip_tensor_data(const snnhip_tensor* t);
size_t snnhip_tensor_bytes(const snnhip_tensor* t);
int snnhip_tensor_dtype(const snnhip_tensor* t);
int snnhip_tensor_upload(snnhip_tensor* t, const float* host_nhwc);          /* H2D, synchronous */
int snnhip_tensor_download(const snnhip_tensor* t, float* host_nhwc);        /* stream sync + D2H */
/* Reference texture layout [ceil(C/4)][H][W][4] per image (shaderUnitTest.cpp:87-129, image.cpp:216-245). */
int snnhip_tensor_upload_c4hw4(snnhip_tensor* t, const float* host_c4hw4);
int snnhip_tensor_download_c4hw4(const snnhip_tensor* t, float* host_c4hw4);
int snnhip_tensor_fill(snnhip_tensor* t, float value);

/* ---- plans ---------------------------------------------------------------------------------------- */

/* Mirror of the conv shaders' 20 specialisation constants (conv2dVulkan.cpp:182-203) plus batch. */
typedef struct {
    int N, H, W, IC, OC;
    int kh, kw, sh, sw;
    int padT, padB, padL, padR; /* getPaddingOffset order; like the reference the kernel offsets x by padT and y
                                   by padL (conv2dVulkan.cpp:183-184) */
    int padMode;                /* SNNHIP_PAD_* ; ignored for 1x1 (vk_conv2d_1x1.comp has no padding) */
    int act;                    /* SNNHIP_ACT_* */
    float leaky;
    int useBias, useBN;
    int dtype;                  /* SNNHIP_F32 | SNNHIP_F16: type of the input and output tensors (weights are given in fp32 and converted) */
    int OH, OW;                 /* 0 => derived with the reference's float rule (conv2d.cpp:102-113) */
} snnhip_conv2d_desc;

/* w_oihw [OC][IC][kh][kw]; bias [OC] or NULL; BN arrays [OC] or NULL (required when useBN). Host pointers.
 * A half-precision layer whose own input or output tensor would have 2^31 or more elements (a layer behind a fused UpSampling2D / Pad, whose nominal
 * input never exists) gets a DESCRIPTION-ONLY plan: snnhip_chain_plan_create fuses from it (graph rule D), snnhip_plan_run on it alone returns
 * SNNHIP_E_UNSUPPORTED with a message. */
int snnhip_conv2d_plan_create(snnhip_ctx* ctx, const snnhip_conv2d_desc* desc, const float* w_oihw, const float* bias,
                              const float* bn_beta, const float* bn_gamma, const float* bn_mean, const float* bn_var,
                              snnhip_plan** out);

/* depthwise: IC == OC == channels, w_chw [C][kh][kw]; zero padding by tap clipping (vk_depthwise.comp:77-78) */
int snnhip_depthwise_plan_create(snnhip_ctx* ctx, const snnhip_conv2d_desc* desc, const float* w_chw, const float* bias,
                                 const float* bn_beta, const float* bn_gamma, const float* bn_mean, const float* bn_var,
                                 snnhip_plan** out);

/* dense activations follow the reference CPU path (cpulayer.h:38-42,199-261) */
enum {
    SNNHIP_DENSE_IDENTITY = 0,
    SNNHIP_DENSE_RELU = 1,
    SNNHIP_DENSE_LEAKY = 2,
    SNNHIP_DENSE_SIGMOID = 3,
    SNNHIP_DENSE_SOFTMAX = 4,
    SNNHIP_DENSE_TANH = 5,
    SNNHIP_DENSE_SILU_NOOP = 6
};
typedef struct {
    int batch, in_units, out_units;
    int act;
    float leaky;
    int useBias;
} snnhip_dense_desc;
/* w_flat: the JSON "kernel" array exactly as stored; read as [Out][In] (cpulayer.h:162, vk_dense.comp:69-72).
 * Input tensor: any NHWC tensor with H*W*C == in_units per image (flatten order HWC, cpulayer.h:94-113).
 * Output tensor: [batch][1][1][out_units]. */
int snnhip_dense_plan_create(snnhip_ctx* ctx, const snnhip_dense_desc* desc, const float* w_flat, const float* bias,
                             snnhip_plan** out);

enum { SNNHIP_SUBPIXEL_D2S = 0, SNNHIP_SUBPIXEL_VK_QUIRK = 1 };
typedef struct {
    int N, H, W, C;
    int factor; /* reference hard-codes 2 (subpixelmerge.h:26-33) */
    int mode;   /* SNNHIP_SUBPIXEL_* ; tanh is always applied (vk_subpixel.comp:64-66) */
} snnhip_subpixel_desc;
int snnhip_subpixel_plan_create(snnhip_ctx* ctx, const snnhip_subpixel_desc* desc, snnhip_plan** out);

/* ---- element-wise, pooling and shape operators next to the conv path: what a ResNet-18 /
 * MobileNetV2 / Candy graph needs between its convolutions.  All are HBM-bound NHWC kernels (16-byte channel-contiguous accesses).
 *   reference interface replaced (core/src/ic2, core/data/assets/shaders)         | entry point
 *   AddLayerVulkan::createCS addlayerVulkan.cpp:33-114 + vk_add.comp:41-88        | snnhip_add_plan_create (two inputs: snnhip_plan_run_n)
 *   ActivationLayerVulkan activationVulkan.cpp + vk_activation.comp:41-86         | snnhip_activation_plan_create
 *   BatchNormalizationLayerVulkan batchnormVulkan.cpp + vk_batchnorm.comp:54-104  | snnhip_batchnorm_plan_create
 *   MaxPooling2DLayerVulkan maxpool2dVulkan.cpp:33-130 + vk_maxpool2d.comp:42-74  | snnhip_pool2d_plan_create (type 0)
 *   AveragePooling2DLayerVulkan avgpool2dVulkan.cpp + vk_avgpool2d.comp:42-69     | snnhip_pool2d_plan_create (type 1)
 *   AdaptiveAvgPool2dLayerGl adaptiveavgpool2dGL.cpp (mean over the whole image)  | snnhip_pool2d_plan_create (type 1, kernel = input size)
 *   PadLayerVulkan padlayerVulkan.cpp:33-110 + vk_pad.comp:42-71                  | snnhip_pad_plan_create
 *   UpSampling2DLayerVulkan upsampling2dVulkan.cpp:35-123 + vk_upsampling2d_{nearest,bilinear}.comp | snnhip_upsample_plan_create
 *   InstanceNormLayerVulkan instancenormVulkan.cpp + vk_instancenorm.comp:53-160  | snnhip_instancenorm_plan_create */
typedef struct {
    int N, H, W, C;
    int act;      /* SNNHIP_ACT_* (0..6; the quirk id 7 is conv-only) */
    float leaky;
} snnhip_eltwise_desc;
/* Add: desc = OUTPUT dims = max over the two inputs (genericlayer.cpp:64-90).  Inputs smaller than that are accepted at run time with the
 * reference's semantics: the sum is evaluated over the first input's extent, the second input reads 0 outside its own (vk_add.comp:47-49) */
int snnhip_add_plan_create(snnhip_ctx* ctx, const snnhip_eltwise_desc* desc, snnhip_plan** out);
int snnhip_activation_plan_create(snnhip_ctx* ctx, const snnhip_eltwise_desc* desc, snnhip_plan** out);
/* y = act(gamma / max(sqrt(var + 1e-3), 1e-4) * (x - mean) + beta), per channel (vk_batchnorm.comp:63-68) */
int snnhip_batchnorm_plan_create(snnhip_ctx* ctx, const snnhip_eltwise_desc* desc, const float* beta, const float* gamma, const float* mean,
                                 const float* var, snnhip_plan** out);

#define SNNHIP_POOL_MAX 0
#define SNNHIP_POOL_AVG 1
typedef struct {
    int N, H, W, C;
    int kh, kw, sh, sw;
    int padT, padL; /* the Vulkan layers force both to 0 ("not padding on top left", maxpool2dVulkan.cpp:62-64); kept as parameters */
    int OH, OW;     /* 0 = derive with the reference's float rule: in/stride + max(0, 1 - k/stride | 1 - 1/stride) (maxpool2d.cpp:26-36) */
    int same;       /* padding mode for the OH/OW rule: 0 "valid"/"none"/"0", 1 anything else */
    int type;       /* SNNHIP_POOL_*: window clipped to the image; max starts at -100000.0, avg divides by the clipped count */
} snnhip_pool2d_desc;
int snnhip_pool2d_plan_create(snnhip_ctx* ctx, const snnhip_pool2d_desc* desc, snnhip_plan** out);

typedef struct {
    int N, H, W, C;
    int padT, padB, padL, padR; /* output = (H + padT + padB) x (W + padL + padR) (padlayer.cpp:58-67) */
    int mode;                   /* 0 constant (zeros), 1 replicate, 2 reflect (vk_pad.comp:55-66) */
} snnhip_pad_desc;
/* reference quirk kept: the shader shifts x by padT and y by padL (padlayerVulkan.cpp:81-82 feeds uPad = {offsets[0], offsets[2]}) */
int snnhip_pad_plan_create(snnhip_ctx* ctx, const snnhip_pad_desc* desc, snnhip_plan** out);

#define SNNHIP_UPSAMPLE_NEAREST 0
#define SNNHIP_UPSAMPLE_BILINEAR 1
typedef struct {
    int N, H, W, C;
    float scale; /* output = trunc(in * scale) (upsampling2d.h:41-44); the shaders sample at pos * (1/scale) */
    int mode;    /* SNNHIP_UPSAMPLE_* */
} snnhip_upsample_desc;
int snnhip_upsample_plan_create(snnhip_ctx* ctx, const snnhip_upsample_desc* desc, snnhip_plan** out);

typedef struct {
    int N, H, W, C;
    int act;
    float leaky;
    float eps; /* the Vulkan shader hard-codes 1e-5 and ignores the parsed epsilon (vk_instancenorm.comp:118); pass 1e-5f for parity */
} snnhip_instancenorm_desc;
/* y = act((x - mean_hw) * gamma / sqrt(var_hw + eps) + beta), statistics per image and channel, biased variance (computed in one sweep
 * around a per-channel pivot: same value as the shader's two-pass form up to fp32 rounding) */
int snnhip_instancenorm_plan_create(snnhip_ctx* ctx, const snnhip_instancenorm_desc* desc, const float* beta, const float* gamma, snnhip_plan** out);

/* ---- the remaining graph operators (U-Net / YOLOv3-tiny concat, unary, transposed convolution, the
 * moonwellbox "Calculate" op) and the device-side step either side of a model run (input resize + normalise, u8 image -> tensor).
 *   reference interface replaced                                                              | entry point
 *   ConcatenateLayerVulkan::createCS concatenationVulkan.cpp:31-88 + vk_concat.comp:39-52      | snnhip_concat_plan_create (two inputs)
 *   UnaryLayerVulkan::createCS unaryVulkan.cpp:30-83 + vk_unary.comp:40-90                     | snnhip_unary_plan_create
 *   Conv2DTransposeLayerGl::createCS deconv2dGL.cpp:282-343 + cs_4x_deconv_2s_RGBA.glsl:150-195 | snnhip_deconv2d_plan_create
 *   CalculateLayerGl::createFS calculationGL.cpp:28-57 + fs_calculation.glsl:25-41            | snnhip_calculate_plan_create
 *   ImageTextureVulkan::resize imageTextureVulkan.cpp:137-183 + vk_resize.comp:41-62           | snnhip_resize_plan_create
 *   snn::normalize / norm2rgba32f image.cpp:712-796 (ImageTexture::convertToRGBA32FAndNormalize) | snnhip_image_u8_plan_create */
typedef struct {
    int N, H, W;
    int C0, C1; /* channels of input 0 / input 1 */
    int OC;     /* the layer's "outputPlanes".  The shader concatenates TEXEL PLANES (4-channel groups), not channels: output plane p comes
                   from input 0 while p < ceil(C0/4), else from input 1's plane p - ceil(C0/4) (vk_concat.comp:43-49).  For C0 % 4 == 0 that
                   is the ordinary channel concat; otherwise input 1 starts at channel 4*ceil(C0/4), the gap reads 0, and whatever does
                   not fit into ceil(OC/4) planes is dropped -- reproduced as is. */
} snnhip_concat_desc;
int snnhip_concat_plan_create(snnhip_ctx* ctx, const snnhip_concat_desc* desc, snnhip_plan** out);

/* vk_unary.comp:46-88 (UnaryDesc::opType is never parsed from JSON, unary.h:27-32: models get 0 = copy) */
enum { SNNHIP_UNARY_COPY = 0, SNNHIP_UNARY_FIXED = 1, SNNHIP_UNARY_NEG = 2, SNNHIP_UNARY_RCP = 3, SNNHIP_UNARY_SQUARE = 4, SNNHIP_UNARY_EXP = 5, SNNHIP_UNARY_ABS = 6 };
typedef struct {
    int N, H, W, C;
    int op;      /* SNNHIP_UNARY_* */
    float value; /* the constant of SNNHIP_UNARY_FIXED */
} snnhip_unary_desc;
int snnhip_unary_plan_create(snnhip_ctx* ctx, const snnhip_unary_desc* desc, snnhip_plan** out);

/* Transposed convolution as the reference's compute shader states it for k=4, s=2 (cs_4x_deconv_2s_RGBA.glsl:150-182): a correlation of the
 * kernel with the zero-stuffed input, zero outside the input (the GL sampler clamps to a transparent border, openGLBackend.cpp:41-43):
 *     y[oy][ox][o] = act(BN(bias[o] + sum_{iy,ix,i} x[iy][ix][i] * w[o][i][(k-1-p) - oy + s*iy][(k-1-p) - ox + s*ix]))   (taps inside the kernel)
 * with p = (k - s) / 2 and output s*H x s*W for "same", p = 0 and s*H + k - s for anything else (deconv2dGL.cpp:345-355).  The desc is the
 * conv desc: kh == kw, sh == sw, padT carries p, padMode / padB / padL / padR are ignored, OH / OW = 0 derives the "same" extent.
 * Activations: relu, tanh, sigmoid, leakyRelu (deconv2dGL.cpp:198-207); BN eps 1e-3 (cs_4x_deconv_2s_RGBA.glsl:190).
 * Pinned against the reference arithmetic for k=4, s=2 only -- the 3x3 / 4x4 stride-1 GL shaders carry sampler-state-dependent texel
 * tests (cs_3x_deconv_RGBA.glsl:77-87) that have no counterpart off the GL rasteriser; other (k, s) follow the formula above. */
int snnhip_deconv2d_plan_create(snnhip_ctx* ctx, const snnhip_conv2d_desc* desc, const float* w_oihw, const float* bias, const float* bn_beta,
                                const float* bn_gamma, const float* bn_mean, const float* bn_var, snnhip_plan** out);

/* fs_calculation.glsl:25-41: y[..][c] = x[..][c % 4] / x[..][8] for c % 4 < 3, else 0 (every 4-channel output pass repeats the same value) */
typedef struct {
    int N, H, W, C; /* C >= 9: the divisor is channel 8 (texel plane 2, .r) */
    int OC;
} snnhip_calculate_desc;
int snnhip_calculate_plan_create(snnhip_ctx* ctx, const snnhip_calculate_desc* desc, snnhip_plan** out);

/* Input pre-processing on the device: resample to OH x OW and normalise, y = (sample(x) - means[c % 4]) * norms[c % 4] (vk_resize.comp:48-60).
 * Sample position of output pixel (x, y): ((x + 0.5) * W / OW, (y + 0.5) * H / OH) in input texel space, clamp-to-edge; linear = the Vulkan
 * bilinear filter with exact fp32 weights (hardware uses 8-bit sub-texel weights: up to 2^-9 of the local range away), else nearest. */
typedef struct {
    int N, H, W, C;
    int OH, OW; /* ImageTextureVulkan::resize: round(W / xScale), round(H / yScale) (imageTextureVulkan.cpp:150-151) */
    float means[4], norms[4];
    int linear;
} snnhip_resize_desc;
int snnhip_resize_plan_create(snnhip_ctx* ctx, const snnhip_resize_desc* desc, snnhip_plan** out);

/* 8-bit image -> normalised 4-channel tensor, the device-side form of convertToRGBA32FAndNormalize (image.cpp:712-751):
 *   src_channels 4 (RGBA8): y[c] = (u8[c] - means[c]) * norms[c];   3 (RGB8): same for c < 3, alpha = 1;
 *   1 (R8): y[0] = (u8 - means[0]) * norms[0], y[1..3] = (0 - means[0]) * norms[0].
 * The input of snnhip_plan_run is a tensor of dtype SNNHIP_U8 [N][H][W][src_channels]; the output is [N][H][W][4] fp32 or fp16. */
typedef struct {
    int N, H, W;
    int src_channels;
    float means[4], norms[4];
} snnhip_image_u8_desc;
int snnhip_image_u8_plan_create(snnhip_ctx* ctx, const snnhip_image_u8_desc* desc, snnhip_plan** out);
/* raw byte upload for SNNHIP_U8 / SNNHIP_U16 tensors (nbytes must equal snnhip_tensor_bytes; 16-bit elements in host byte order) */
int snnhip_tensor_upload_raw(snnhip_tensor* t, const void* host, size_t nbytes);
/* raw byte download (any dtype; nbytes must equal snnhip_tensor_bytes): stream sync + D2H, the counterpart of snnhip_tensor_upload_raw */
int snnhip_tensor_download_raw(const snnhip_tensor* t, void* host, size_t nbytes);

/* 8-bit frames at both ends of a model.  Unlike snnhip_image_u8_plan_create these keep the channel count (no widening to RGBA).
 *   u8_in :  U8 [N][H][W][C] -> dtype [N][H][W][C],   y = (float(u) - means[c]) * norms[c]      (a subtract, then a multiply: no fma)
 *   u8_out:  dtype [N][H][W][C] -> U8 [N][H][W][C],   q = clamp(rint(fmaf(x, scale[c], offset[c])), 0, 255)
 * The u8_out contract: fmaf in fp32 (an fp16 input is widened exactly first), rounding to nearest with ties to even, NaN -> 0, +inf -> 255,
 * -inf -> 0.  It is the single definition: the chain rules that fold these plans into the ESPCN kernels (A8: u8_in with C == 1 and dtype F32 in
 * front of rule A; B8: u8_out with C == 1 behind rule B) reproduce both maps bit for bit, out-of-image taps of kernel A staying 0 in the
 * NORMALISED domain, exactly as the separate launches give them.  C is 1..4; dtype SNNHIP_F32 or SNNHIP_F16. */
typedef struct {
    int N, H, W, C;
    int dtype;
    float means[4], norms[4];
} snnhip_u8_in_desc;
int snnhip_u8_in_plan_create(snnhip_ctx* ctx, const snnhip_u8_in_desc* desc, snnhip_plan** out);
typedef struct {
    int N, H, W, C;
    int dtype;
    float scale[4], offset[4];
} snnhip_u8_out_desc;
int snnhip_u8_out_plan_create(snnhip_ctx* ctx, const snnhip_u8_out_desc* desc, snnhip_plan** out);

/* 16-bit frames at both ends of a model: 10-, 12- and 16-bit video in 2-byte unsigned containers (SNNHIP_U16), channel count kept.
 *   u16_in :  U16 [N][H][W][C] -> dtype [N][H][W][C],   y = (float(u >> shift) - means[c]) * norms[c]      (a subtract, then a multiply: no fma;
 *             an fp16 output rounds that fp32 value to nearest even)
 *   u16_out:  dtype [N][H][W][C] -> U16 [N][H][W][C],   q = unsigned(clamp(rint(fmaf(x, scale[c], offset[c])), 0, maxval)) << shift
 * The u16_out contract: fmaf in fp32 (an fp16 input is widened exactly first), rounding to nearest with ties to even, NaN -> 0,
 * +inf -> maxval << shift, -inf -> 0.  It is the single definition of the 16-bit maps.  `shift` and `maxval` name the container layout:
 *   low-aligned 10 / 12-bit (yuv420p10le, gray12le):   maxval 1023 / 4095,  shift 0
 *   high-aligned 10-bit (P010: value in the top bits): maxval 1023,         shift 6
 *   full 16-bit:                                       maxval 65535,        shift 0
 * u16_in ignores the bits below `shift`; u16_out writes them as 0.  C is 1..4; dtype SNNHIP_F32 or SNNHIP_F16; shift 0..15.  u16_out_plan_create
 * returns SNNHIP_E_INVALID with a message unless 1 <= maxval <= 65535 and (maxval << shift) <= 65535.  The chain planner folds both into the fused
 * ESPCN kernels (C == 1, dtype = the launch's own: the fp32 kernels, and the fp16 ones under SNNHIP_ESPCN_F16=1; at the chain's ends), bit for bit what the separate launches give, out-of-image taps
 * of kernel A staying 0 in the NORMALISED domain; every other chain runs them as launches of their own. */
typedef struct {
    int N, H, W, C;
    int dtype;
    float means[4], norms[4];
    int shift;
} snnhip_u16_in_desc;
int snnhip_u16_in_plan_create(snnhip_ctx* ctx, const snnhip_u16_in_desc* desc, snnhip_plan** out);
typedef struct {
    int N, H, W, C;
    int dtype;
    float scale[4], offset[4];
    int maxval, shift;
} snnhip_u16_out_desc;
int snnhip_u16_out_plan_create(snnhip_ctx* ctx, const snnhip_u16_out_desc* desc, snnhip_plan** out);

/* Colour frames around a luma-only model (ESPCN, like the reference's demo/modelInferenceESPCN.py, takes and returns the Y plane only): the luma
 * split in front of the model and the chroma merge behind it, on interleaved 8-bit RGB (C = 3) or RGBA (C = 4) frames.  DESIGN.md section 4.13.
 * The arithmetic contract, stated once:
 *   Matrix: full-range Y'CbCr with coefficients kr, kb of the desc and kg = 1 - kr - kb, computed in double and rounded to float.  BT.601 is
 *     kr = 0.299, kb = 0.114 (what cv2.COLOR_BGR2YCrCb uses); BT.709 is 0.2126 / 0.0722.  Limited range is not offered on this RGB-in path; video
 *     sources (NV12 / P010, limited range almost always) go through snnhip_yuv_rgb_plan_create below, which takes either range, and an RGB frame
 *     leaves as limited-range NV12 through snnhip_rgb_cbcr_plan_create.
 *   rgb_luma:   U8 [N][H][W][C] -> U8 [N][H][W][1].  ylo = kr*R + kg*G + kb*B in fp32, q = clamp(rint(ylo), 0, 255), ties to even: the U8 luma plane
 *     that snnhip_u8_in_plan_create (and chain rule A8) consumes unchanged.
 *   ycc_merge:  inputs[0] = Yhi, U8 [N][r*H][r*W][1]; inputs[1] = the original low-resolution frame, U8 [N][H][W][C]; output U8 [N][r*H][r*W][C]
 *     (snnhip_plan_run_n, 2 inputs).  r follows from the two shapes: an integer 1..4, the same on both axes (and the desc's r), else
 *     SNNHIP_E_INVALID with a message.  No quantised CbCr plane exists anywhere: per low-resolution pixel ylo as above, unquantised (one device
 *     function serves both plans), dR = R - ylo, dB = B - ylo.  dR~, dB~ are dR, dB resampled to the output grid with aligned pixel centres: output
 *     column X samples sx = (X + 0.5) / r - 0.5 (rows likewise); i0 = floor(sx), t = sx - i0, taps at i0 - 1 .. i0 + 2 with indices clamped to
 *     [0, W - 1] (replicate edge), weights the Keys cubic with a = -0.5 (Catmull-Rom) at distances 1 + t, t, 1 - t, 2 - t.  An integer r has
 *     exactly r phases: the [r][4] weight table (row p = phase X mod r) is computed on the host in double, rounded to fp32 and handed to the
 *     kernel (snnhip_bicubic_taps returns it).  The filter is separable: horizontal, then vertical.  Then
 *         R' = Yhi + dR~,   B' = Yhi + dB~,   G' = Yhi - (kr*dR~ + kb*dB~) / kg,   q = clamp(rint(.), 0, 255)
 *     and, for C = 4, the alpha byte of the low-resolution pixel (Y / r, X / r) (integer division), copied.
 *   Consequences: a grey frame (R = G = B) comes out as R' = G' = B' = Yhi byte for byte; in fp32 the value in front of the rounding stays within
 *     about 5e-5 of a float64 evaluation (fma contraction moves it by the same order).
 * Both plans read and write SNNHIP_U8 tensors only (a float tensor at any position is refused by snnhip_plan_run_n); plan creation returns
 * SNNHIP_E_INVALID with a message unless C is 3 or 4, r is 1..4 and 0 < kr, 0 < kb, kr + kb < 1.  snnhip_plan_cost reports the bytes each moves:
 * every input once and the output once. */
typedef struct { int N, H, W, C; float kr, kb; } snnhip_rgb_luma_desc;
int snnhip_rgb_luma_plan_create(snnhip_ctx* ctx, const snnhip_rgb_luma_desc* desc, snnhip_plan** out);
typedef struct { int N, H, W, C; int r; float kr, kb; } snnhip_ycc_merge_desc; /* H, W: the LOW-resolution frame */
int snnhip_ycc_merge_plan_create(snnhip_ctx* ctx, const snnhip_ycc_merge_desc* desc, snnhip_plan** out); /* run with snnhip_plan_run_n, 2 inputs */
/* host only, no context (like snnhip_espcn_f16_pack_weights): the [r][4] fp32 tap table the merge kernel uses, r = 1..4, capacity >= 4*r floats */
int snnhip_bicubic_taps(int r, float* out, int capacity);

/* The chroma plane of a 4:2:0 video frame upsampled beside a luma-only model (NV12 / P010 from a hardware decoder: a full-resolution luma plane,
 * which the 8 / 16-bit frame ends above already take, and a half-resolution chroma plane, which this plan takes).  DESIGN.md section 4.14.
 * The contract, stated once:
 *   Shapes: the input is a chroma plane [N][H][W][C] -- C = 2: interleaved CbCr (NV12 / P010), C = 1: one plane of a planar format (I420,
 *     yuv420p10le) -- of dtype SNNHIP_U8 or SNNHIP_U16; H, W are the CHROMA plane's extent.  The output is [N][r*H][r*W][C] of the same dtype,
 *     r = 1..4.  Channels never mix.
 *   Value: v = float(u >> shift) (shift = 0 for SNNHIP_U8).  The filter is ycc_merge's: the Keys cubic with a = -0.5, separable, horizontal then
 *     vertical, indices clamped to the plane (replicate edge), fp32 weights computed on the host in double and rounded to float, fp32
 *     accumulation.  q = unsigned(clamp(rint(.), 0, maxval)) << shift, ties to even.  At r = 1 the output is the input with the bits below
 *     `shift` cleared (for values up to maxval).
 *   Siting: output sample r*x + p reads source position x + s.  The vertical axis always uses aligned sample centres, s = (p + 0.5) / r - 0.5
 *     (scaling a 4:2:0 plane by an integer about aligned centres keeps vertically centred chroma centred).  The horizontal axis follows `siting`:
 *     SNNHIP_SITING_CENTRE is the same phase (JPEG / MPEG-1 siting); SNNHIP_SITING_LEFT is chroma co-sited with the even luma columns (the
 *     default of H.264 / HEVC / AV1 streams, hence of NV12 / P010 from decoders), s = (p + 0.25) / r - 0.25: chroma sample i sits at luma column
 *     2i, output chroma sample j at output luma column 2j = low-resolution luma column (2j + 0.5) / r - 0.5, which halved is chroma index
 *     j / r + 0.25 / r - 0.25.  Taps are floor(s) - 1 .. floor(s) + 2 relative to x; floor(s) (the phase's base, -1 or 0) travels with the
 *     weights; the reach is x - 2 .. x + 2.
 *   Bit depth: maxval is at most 255 for SNNHIP_U8 and at most 4095 for SNNHIP_U16 (10-bit: 1023, 12-bit: 4095); shift is 0, or 16 - bits for the
 *     high-aligned containers (P010: maxval 1023, shift 6); maxval << shift must fit the container.  maxval > 4095 is refused: on full 16-bit values
 *     the fp32 filter is 1.5e-2 away from its float64 value, too far for a rounding contract (P016 chroma is not built).
 * Plan creation returns SNNHIP_E_INVALID with a message for C outside {1, 2}, r outside 1..4, a dtype that is neither SNNHIP_U8 nor SNNHIP_U16, a
 * maxval / shift that does not fit the container and an unknown siting; snnhip_plan_run for a tensor of another dtype at either end and an output
 * that is not r times the input.  snnhip_plan_describe: "chroma_up_u8 r=2 c=2 siting=left tile=8x256 ...".  snnhip_plan_cost counts the input once
 * and the output once.  The reference has nothing for this: core/inc/snn/color.h only enumerates YUV layouts, and the libyuv it vendors scales planes
 * on the CPU with box / bilinear filters. */
#define SNNHIP_SITING_CENTRE 0
#define SNNHIP_SITING_LEFT 1
typedef struct { int N, H, W, C; int r; int dtype; int maxval, shift; int siting; } snnhip_chroma_up_desc; /* H, W: the chroma plane */
int snnhip_chroma_up_plan_create(snnhip_ctx* ctx, const snnhip_chroma_up_desc* desc, snnhip_plan** out); /* run with snnhip_plan_run */
/* host only, no context: the tap table of the horizontal axis (and, with SNNHIP_SITING_CENTRE, of the vertical one): weights [r][4] (capacity >= 4*r
 * floats) and base [r] ints; phase p reads x + base[p] - 1 .. x + base[p] + 2.  With SNNHIP_SITING_CENTRE the weights are snnhip_bicubic_taps' and
 * base is its phase start.  The reference has no counterpart (its libyuv scalers are bilinear / box). */
int snnhip_bicubic_taps_sited(int r, int siting, float* weights, int* base, int capacity);

/* A 4:2:0 video frame to packed RGB behind a luma-only model: the model's upscaled luma frame and the ORIGINAL half-resolution CbCr plane in, RGB or
 * RGBA at the output resolution out, in one launch.  No upscaled chroma plane is written to memory.  DESIGN.md section 4.15.  The contract, stated once:
 *   Shapes: inputs[0] = Yhi [N][2rH][2rW][1], the model's output luma frame; inputs[1] = the original chroma plane [N][H][W][2], interleaved CbCr
 *     (H, W of the desc are the CHROMA plane's extent); output [N][2rH][2rW][C], C = 3 (R, G, B) or 4 (R, G, B, A with A = maxval << shift); run with
 *     snnhip_plan_run_n, 2 inputs.  All three have the same dtype, SNNHIP_U8 or SNNHIP_U16.  r = 1..4; r = 1 is plain NV12 -> RGB with no model in
 *     between.  Values are float(u >> shift).
 *   Chroma filter: the Keys cubic of ycc_merge and chroma_up (a = -0.5), separable, horizontal then vertical, indices clamped to the plane, fp32
 *     weights computed on the host in double and rounded to float, fp32 accumulation.  The chroma grid is resampled straight to the output luma
 *     grid, R = 2r-fold: output column X = R*x + p reads chroma position x + s, s = (p + 0.5) / R - off, off = 0.5 for SNNHIP_SITING_CENTRE and
 *     0.25 for SNNHIP_SITING_LEFT (chroma sample i is co-sited with low-resolution luma column 2i; output luma column X sits at low-resolution
 *     position (X + 0.5) / r - 0.5, which halved is chroma index (X + 0.5) / R - 0.25).  This is NOT chroma_up's left phase, whose output is itself
 *     a chroma grid.  The vertical axis always uses off = 0.5, as chroma_up does.  base = floor(s) is -1 or 0 and travels with the weights; taps are
 *     x + base - 1 .. x + base + 2, the reach x - 2 .. x + 2.  What is filtered is the sample minus Coff (an exact fp32 difference of integers), so
 *     Cb~ - Coff and Cr~ - Coff below are the filter's results themselves.
 *   Matrix: k = (maxval + 1) / 256.  SNNHIP_RANGE_LIMITED: Yoff = 16k, Yrange = 219k, Coff = 128k, Crange = 224k.  SNNHIP_RANGE_FULL: Yoff = 0,
 *     Yrange = maxval, Coff = 128k, Crange = maxval.  kg = 1 - kr - kb.  Five coefficients, computed in double and rounded to float:
 *         cy = maxval / Yrange,  crv = 2(1 - kr) maxval / Crange,  cbu = 2(1 - kb) maxval / Crange,  cgv = kr crv / kg,  cgu = kb cbu / kg
 *     Per output pixel, in fp32:  yl = cy (Y - Yoff),  R = yl + crv (Cr~ - Coff),  B = yl + cbu (Cb~ - Coff),
 *         G = yl - (cgv (Cr~ - Coff) + cgu (Cb~ - Coff)),  q = unsigned(clamp(rint(.), 0, maxval)) << shift, ties to even.
 *     The output is always full-range RGB.
 *   Consequences: neutral chroma (both samples equal to Coff) gives R = G = B = the quantised yl, byte for byte; constant chroma planes give
 *     constant chroma terms.  In fp32 the value in front of the rounding stays within 3e-5 / 1.1e-4 / 5.2e-4 (8 / 10 / 12 bits) of a float64 evaluation.
 * Plan creation returns SNNHIP_E_INVALID with a message for C outside {3, 4}, r outside 1..4, a dtype that is neither SNNHIP_U8 nor SNNHIP_U16,
 * maxval above 255 (U8) or above 4095 (U16, as for chroma_up), a maxval << shift that does not fit the container, maxval + 1 not a multiple of 256,
 * an unknown siting or range and kr, kb outside 0 < kr, 0 < kb, kr + kb < 1; snnhip_plan_run_n for a tensor of another dtype at any position and for
 * shapes that are not 2r times the chroma plane.  snnhip_plan_describe: "yuv_rgb_u8 r=2 c=3 siting=left range=limited tile=8x128 ... kernel=
 * yuv_rgb_kernel" (the tile in chroma pixels).  snnhip_plan_cost counts both inputs once and the output once.  The reference has nothing for this:
 * core/inc/snn/color.h only enumerates YUV layouts, and the libyuv it vendors converts on the CPU. */
#define SNNHIP_RANGE_LIMITED 0
#define SNNHIP_RANGE_FULL 1
typedef struct { int N, H, W, C; int r; int dtype; int maxval, shift; int siting; int range; float kr, kb; } snnhip_yuv_rgb_desc; /* H, W: the CHROMA plane */
int snnhip_yuv_rgb_plan_create(snnhip_ctx* ctx, const snnhip_yuv_rgb_desc* desc, snnhip_plan** out); /* run with snnhip_plan_run_n, 2 inputs */
/* host only, no context: the tap table of the plan's horizontal axis (and, with SNNHIP_SITING_CENTRE, of its vertical one): weights [2r][4]
 * (capacity >= 8*r floats) and base [2r] ints; phase p = X mod 2r reads x + base[p] - 1 .. x + base[p] + 2 */
int snnhip_bicubic_taps_420(int r, int siting, float* weights, int* base, int capacity);
/* host only, no context: out[0..6] = Yoff, Coff, cy, crv, cbu, cgv, cgu of the matrix above (capacity >= 7 floats) */
int snnhip_yuv_rgb_coefficients(int maxval, int range, float kr, float kb, float* out, int capacity);

/* RGB frames in, NV12 out around a luma-only model: the chroma plane of the UPSCALED 4:2:0 frame from the ORIGINAL low-resolution RGB frame, in one
 * launch (capture, upscale, then encode: a hardware encoder takes NV12).  The luma plane of that frame is the model's own 8-bit output (rgb_luma in
 * front, the output map scale 219 / offset 16 for limited range, 255 / 0 for full).  DESIGN.md section 4.17.  The contract, stated once:
 *   Shapes: the input is U8 [N][H][W][C], C = 3 (R, G, B) or 4 (alpha is ignored); H, W are the LOW-resolution frame's.  The output is U8
 *     [N][rH/2][rW/2][2], interleaved Cb, Cr: the chroma plane of an NV12 frame of rH x rW.  r = 2, 3, 4, and rH and rW must be even (r = 3 needs
 *     even H and W).  r = 1 is refused: it would halve the chroma grid, which needs a decimation filter, and is not built.  16-bit sources (RGB16 ->
 *     P010) need a 16-bit luma split that does not exist either.
 *   Chroma differences: per low-resolution pixel ylo = kr R + kg G + kb B in fp32, unquantised (the one device function of rgb_luma and ycc_merge,
 *     kg = 1 - kr - kb as there), dB = B - ylo, dR = R - ylo.
 *   Resampling: the Keys cubic of the plans above (a = -0.5), separable, horizontal then vertical, indices clamped to the frame, fp32 weights computed
 *     on the host in double and rounded to float, fp32 accumulation.  Output chroma column I sits at output luma position 2I for SNNHIP_SITING_LEFT
 *     and midway between columns 2I and 2I + 1 for SNNHIP_SITING_CENTRE: it reads low-resolution position sx = (2I + lead) / r - 0.5, lead = 0.5
 *     (left) or 1.0 (centre).  Rows always use the centre form, as chroma_up and yuv_rgb do.  With g = gcd(r, 2) the pattern repeats every P = r / g
 *     outputs over S = 2 / g inputs ((P, S) = (1, 1), (3, 2), (2, 1) for r = 2, 3, 4): output I = P x' + p reads S x' + s_p, s_p = (2p + lead) / r -
 *     0.5; base_p = floor(s_p) lies in {-1, 0, 1} and travels with the weights; taps are S x' + base_p - 1 .. S x' + base_p + 2.  r = 2 centre is the
 *     identity (s = 0, weights 0, 1, 0, 0), r = 2 left a quarter-pixel shift (s = -0.25), r = 3 left phase 2 the identity on input 2x' + 1.
 *   Matrix: Coff = 128; Crange = 224 for SNNHIP_RANGE_LIMITED, 255 for SNNHIP_RANGE_FULL; cbs = Crange / (2 (1 - kb) 255), crs = Crange /
 *     (2 (1 - kr) 255), computed in double and rounded to float: the inverses of yuv_rgb's cbu and crv.  Cb = Coff + cbs dB~, Cr = Coff + crs dR~,
 *     q = clamp(rint(.), 0, 255), ties to even.
 *   Consequences: a grey frame (R = G = B) gives Cb = Cr = 128 byte for byte; a constant frame gives a constant plane; at r = 2 centre the plane is
 *     the per-pixel conversion of the input.  In fp32 the value in front of the rounding stays within 2.6e-5 of a float64 evaluation (measured; the
 *     worst case of the expression, sixteen roundings at half an ulp of 256, is 2.4e-4).
 * Plan creation returns SNNHIP_E_INVALID with a message for C outside {3, 4}, r outside 2..4, an odd rH or rW, an unknown siting or range and kr, kb
 * outside 0 < kr, 0 < kb, kr + kb < 1; snnhip_plan_run for a tensor that is not SNNHIP_U8 at either end and an output that is not [N][rH/2][rW/2][2].
 * snnhip_plan_describe: "rgb_cbcr_u8 r=2 c=3 siting=left range=limited tile=8x256 ... kernel=rgb_cbcr_kernel" (the tile in output chroma pixels).
 * snnhip_plan_cost counts the input once and the output once.  The reference has nothing for this (its ESPCN demo writes a grey image). */
typedef struct { int N, H, W, C; int r; int siting; int range; float kr, kb; } snnhip_rgb_cbcr_desc; /* H, W: the LOW-resolution RGB frame */
int snnhip_rgb_cbcr_plan_create(snnhip_ctx* ctx, const snnhip_rgb_cbcr_desc* desc, snnhip_plan** out); /* run with snnhip_plan_run */
/* host only, no context: the tap table of the plan's horizontal axis (and, with SNNHIP_SITING_CENTRE, of its vertical one): weights [P][4] (capacity
 * >= 4 * P floats, P = 1, 3, 2 for r = 2, 3, 4) and base [P] ints; phase p reads S x' + base[p] - 1 .. S x' + base[p] + 2 */
int snnhip_bicubic_taps_rgb420(int r, int siting, float* weights, int* base, int capacity);
/* host only, no context: out[0..2] = Coff, cbs, crs of the matrix above (capacity >= 3 floats) */
int snnhip_rgb_cbcr_coefficients(int range, float kr, float kb, float* out, int capacity);

/* Planar 4:2:0 chroma (I420 / I010: ffmpeg's yuv420p / yuv420p10le, what software decoders write and software encoders read) for the two plans above
 * that touch BOTH chroma components.  DESIGN.md section 4.19.  The contract, stated once:
 *   The planar chroma tensor is [2N][H][W][1] of dtype SNNHIP_U8 or SNNHIP_U16: plane 2n is the Cb plane of image n, plane 2n + 1 its Cr plane, each
 *     dense.  (A YV12 caller swaps the two planes when it copies them in or out.)
 *   snnhip_yuv_rgb_planar_plan_create takes snnhip_yuv_rgb_desc unchanged.  inputs[0] = Yhi [N][2rH][2rW][1], inputs[1] = the planar chroma tensor
 *     [2N][H][W][1]; output [N][2rH][2rW][C].  Output, arithmetic, tap tables and coefficients are exactly those of snnhip_yuv_rgb_plan_create on
 *     the interleaved plane with the same samples (r = 1..4, C = 3 | 4, 8 / 10 / 12 bits, high-aligned containers, either range and siting); so are
 *     the refusals at plan creation.  snnhip_plan_run_n refuses, with a message starting "yuv_rgb_planar", a tensor of another dtype at any position,
 *     a chroma tensor that is not [2N][H][W][1] and shapes that are not 2r times a chroma plane.  snnhip_plan_describe: "yuv_rgb_planar_u8 r=2 c=3 ...
 *     kernel=yuv_rgb_planar_kernel", the tile that of the interleaved plan.
 *   snnhip_rgb_cbcr_planar_plan_create takes snnhip_rgb_cbcr_desc unchanged.  Input U8 [N][H][W][C]; output U8 [2N][rH/2][rW/2][1], r = 2..4; the
 *     arithmetic and the refusals at plan creation (r = 1 among them) are those of snnhip_rgb_cbcr_plan_create.  snnhip_plan_run refuses, with a message
 *     starting "rgb_cbcr_planar", a tensor that is not SNNHIP_U8 and an output that is not [2N][rH/2][rW/2][1].  snnhip_plan_describe:
 *     "rgb_cbcr_planar_u8 r=2 c=3 ... kernel=rgb_cbcr_planar_kernel".
 *   Both are one launch: no interleaved plane is formed anywhere, and no LDS, barrier or scratch is used.  Every byte of both output planes (of the RGB
 *     frame) is written.  Planar in, planar out needs no plan of its own: snnhip_chroma_up_plan_create and snnhip_plane_fit_plan_create with C = 1
 *     and N = 2 * batch run over the planar chroma tensor. */
int snnhip_yuv_rgb_planar_plan_create(snnhip_ctx* ctx, const snnhip_yuv_rgb_desc* desc, snnhip_plan** out); /* run with snnhip_plan_run_n, 2 inputs */
int snnhip_rgb_cbcr_planar_plan_create(snnhip_ctx* ctx, const snnhip_rgb_cbcr_desc* desc, snnhip_plan** out); /* run with snnhip_plan_run */

/* A plane resampled to any size between half and four times its own, each axis with its own ratio: what brings the r-fold frame of the luma model
 * (and the original chroma plane beside it) to the size a pipeline asks for -- 720p to 1080p is the x2 model, then 3/4.  The plans above change a
 * frame's size by the model's factor only.  DESIGN.md section 4.18.  The contract, stated once:
 *   Shapes: the input is a plane [N][H][W][C] of dtype SNNHIP_U8 or SNNHIP_U16, C = 1 (a luma plane, a grey frame, one plane of a planar chroma
 *     format) or C = 2 (interleaved CbCr); the output is [N][OH][OW][C] of the same dtype.  Channels never mix.  Values are float(u >> shift), maxval
 *     and shift as for chroma_up (maxval <= 4095).
 *   Phase: separable, each axis on its own.  Along an axis with I inputs and O outputs, output X reads source position s = (X + lead) I / O - off.
 *     The vertical axis, and a horizontal axis with SNNHIP_SITING_CENTRE, use lead = off = 1/2 (aligned centres; a luma plane always does); a
 *     horizontal axis with SNNHIP_SITING_LEFT uses lead = off = 1/4: the output is a chroma grid of the same siting, as in chroma_up.  In integers,
 *     so that every implementation gets the same base: a = 4 lead (2 or 1), Nn = (4X + a) I - a O, D = 4 O, base = floor(Nn / D),
 *     t = (Nn - base D) / D.
 *   Weights: eight taps at base - 3 .. base + 4, tap k at distance |k - 3 - t|, weight keys_cubic(distance * f) with the Keys cubic of the plans
 *     above (a = -0.5) and f = min(O / I, 1): the kernel is stretched when shrinking (the anti-aliasing low-pass) and is the plain four-tap cubic
 *     when enlarging, where the outer four weights are exactly 0.  The eight are summed in ascending tap order in double, divided by that sum and
 *     rounded to float.  Source indices clamp to the plane (replicate edge).  fp32 accumulation, vertical then horizontal;
 *     q = unsigned(clamp(rint(.), 0, maxval)) << shift, ties to even.
 *   Ratios: 1/2 <= O / I <= 4 on each axis (eight taps are exactly enough at 1/2); everything else is refused.
 *   Consequences: O == I on an axis gives base = X, t = 0 and weights (0, 0, 0, 1, 0, 0, 0, 0): that axis copies, and with both the output is the
 *     input with the bits below `shift` cleared.  For O = r I the inner four weights are snnhip_bicubic_taps_sited's row of phase X mod r (to one
 *     float ulp: the division by a sum that is 1 to 1e-16) with the same bases.  A constant plane stays constant.  In fp32 the value in front of
 *     the rounding stays within 4.6e-5 / 2.1e-4 / 7.3e-4 (8 / 10 / 12 bits) of a float64 evaluation.
 * Plan creation returns SNNHIP_E_INVALID with a message starting "plane_fit desc" for C outside {1, 2}, a ratio outside [1/2, 4] on either axis (the
 * message names the axis and both extents), bad dims, and dtype, maxval, shift and siting as chroma_up does; snnhip_plan_run for a tensor of another
 * dtype or shape at either end.  snnhip_plan_describe: "plane_fit_u8 c=2 1440x2560->1080x1920 siting=left tile=22x128 taps=8 ... kernel=
 * plane_fit_kernel" (the tile in output pixels).  snnhip_plan_cost counts the input once and the output once.
 * RGB output at a fitted size and fitted RGB8 colour frames are snnhip_rgb_fit_plan_create below, behind this plan with C = 1 on the luma frame.
 * Not built: ratios below 1/2 (they need more than eight taps); the host mirror (include/snn_c.h, snn_model_create11) puts this plan behind
 * NV12 / P010 models only, grey frames go through the plan itself.  The reference has
 * nothing for this: the libyuv it vendors scales planes on the CPU with box / bilinear filters. */
typedef struct { int N, H, W, C; int OH, OW; int dtype; int maxval, shift; int siting; } snnhip_plane_fit_desc;
int snnhip_plane_fit_plan_create(snnhip_ctx* ctx, const snnhip_plane_fit_desc* desc, snnhip_plan** out); /* run with snnhip_plan_run */
/* host only, no context: the table of one axis with `in` inputs and `out` outputs: weights [out][8] (capacity >= 8 * out floats) and base [out]
 * ints; output X reads in[clamp(base[X] - 3 + k)] with weights[X][k], k = 0..7.  The plan builds its two tables with this function (the vertical
 * one with SNNHIP_SITING_CENTRE) and keeps them in device memory.  SNNHIP_E_INVALID with a message for a ratio outside [1/2, 4], a null pointer,
 * too little room and an unknown siting. */
int snnhip_fit_taps(int in, int out, int siting, float* weights, int* base, int capacity);

/* Packed RGB at any output size behind a luma-only model: the luma frame ALREADY at the output size (the model's r-fold frame through
 * snnhip_plane_fit_plan_create with C = 1, centre) and the ORIGINAL low-resolution chroma source in, RGB or RGBA at the output size out, in one
 * launch -- 720p to 1080p through the x2 or the x3 model, 1080p to 1440p.  No r-fold chroma plane and no r-fold RGB frame exists anywhere.  The two
 * fixed-phase RGB sinks above (yuv_rgb, ycc_merge) keep r or 2r phases in registers and cannot take a table per coordinate; this plan has
 * plane_fit's shape.  DESIGN.md section 4.24.  The contract, stated once:
 *   Shapes: inputs[0] = Yfit [N][OH][OW][1]; inputs[1] = the chroma source, by `source`; output [N][OH][OW][C], C = 3 (R, G, B) or 4 (+ A); run
 *     with snnhip_plan_run_n, 2 inputs.  H, W of the desc are the chroma source's extent: the chroma plane's for the two video sources, the
 *     low-resolution frame's for SNNHIP_RGB_FIT_RGB.  The source is only ever enlarged: a 4:2:0 chroma plane 2r/2 .. 2r-fold, an RGB frame 1 .. r-fold.
 *   Phase: separable, each axis with its own ratio, 1 <= O / I <= 8.  Output X reads source position s = (X + 1/2) I / O - off: the output is a luma
 *     grid.  off = 1/2 on the vertical axis, on a horizontal axis with SNNHIP_SITING_CENTRE and always for SNNHIP_RGB_FIT_RGB; off = 1/4 on the
 *     horizontal axis of a left-sited 4:2:0 plane (chroma sample i sits at luma column 2i): yuv_rgb's phase to the luma grid, NOT plane_fit's to a
 *     chroma grid.  In integers: a = 4 off (2 or 1), Nn = (4X + 2) I - a O, D = 4 O, base = floor(Nn / D), t = (Nn - base D) / D.
 *   Weights: plane_fit's rule with f = 1: the eight Keys values (a = -0.5) at |k - 3 - t| summed in ascending order in double, each divided by the
 *     sum and rounded to float.  The outer four are exactly 0; the table keeps the inner four, taps at base - 1 .. base + 2, indices clamped to the
 *     source (replicate edge).  Vertical, then horizontal, fp32 accumulation.
 *   Video sources (SNNHIP_RGB_FIT_CBCR, SNNHIP_RGB_FIT_PLANAR): everything is yuv_rgb's.  Values are float(u >> shift); what is filtered is the
 *     sample minus Coff; the five coefficients are snnhip_yuv_rgb_coefficients'; per output pixel yl = cy (Yfit - Yoff), R = yl + crv Cr~,
 *     B = yl + cbu Cb~, G = yl - (cgv Cr~ + cgu Cb~), full-range RGB, q = unsigned(clamp(rint(.), 0, maxval)) << shift, A = maxval << shift.  Yfit
 *     and the output have the chroma tensor's dtype (SNNHIP_U8 or SNNHIP_U16, maxval <= 4095, maxval + 1 a multiple of 256).
 *   RGB source (SNNHIP_RGB_FIT_RGB, SNNHIP_U8 only; maxval, shift, siting and range of the desc are not read): everything is ycc_merge's.  Per
 *     low-resolution pixel the unquantised ylo (the one device function of rgb_luma and ycc_merge), dR = R - ylo, dB = B - ylo, resampled;
 *     R' = Yfit + dR~, B' = Yfit + dB~, G' = Yfit - (kr dR~ + kb dB~) / kg, q = clamp(rint(.), 0, 255); for C = 4 the alpha byte of source pixel
 *     ((2Y + 1) H / (2 OH), (2X + 1) W / (2 OW)) by integer division (at OH = rH that is ycc_merge's Y / r).
 *   Consequences: for O = 2r I the table is snnhip_bicubic_taps_420's row X mod 2r and for O = r I (centre) snnhip_bicubic_taps' row X mod r, with
 *     the same bases and the weights to one float ulp (the division by a sum that is 1 to 1e-15).  O == I with off = 1/2 gives base = X and weights
 *     (0, 1, 0, 0).  Neutral chroma, or a grey source frame, gives R = G = B = the quantised luma term, byte for byte; constant chroma planes give
 *     constant chroma terms.  In fp32 the value in front of the rounding stays within 2.7e-5 / 1.2e-4 / 4.6e-4 (video, 8 / 10 / 12 bits) and 6.3e-5
 *     (RGB source, whole-range bytes) of a float64 evaluation (measured: tests/rgb_fit_ref.py).
 * Plan creation returns SNNHIP_E_INVALID with a message starting "rgb_fit desc" for bad dims, C outside {3, 4}, an unknown source, a ratio outside
 * [1, 8] on either axis (the message names the axis and both extents), the RGB source with a dtype other than SNNHIP_U8, and for the video sources
 * everything yuv_rgb refuses about dtype, maxval, shift, siting and range; kr, kb outside 0 < kr, 0 < kb, kr + kb < 1 for every source.  It also
 * checks what the kernel relies on -- bases never step back, no tile's source span exceeds its LDS rows -- and refuses otherwise.
 * snnhip_plan_run_n refuses a tensor of another dtype or shape at any position.  snnhip_plan_describe: "rgb_fit_u8 src=cbcr c=3 360x640->1080x1920
 * siting=left range=limited tile=22x256 taps=4 lds=49152 ... kernel=rgb_fit_kernel" (the tile in output pixels).  snnhip_plan_cost counts both
 * inputs once and the output once.  Not built: a fused luma fit (three float planes through LDS), RGB16 sources, BGR order, 4:2:2 / 4:4:4.  The
 * reference has nothing for this: the libyuv it vendors scales and converts on the CPU. */
#define SNNHIP_RGB_FIT_CBCR 0   /* inputs[1] = [N][H][W][2] interleaved CbCr (NV12 / P010) */
#define SNNHIP_RGB_FIT_PLANAR 1 /* inputs[1] = [2N][H][W][1], plane 2n = Cb, 2n + 1 = Cr (I420 / I010) */
#define SNNHIP_RGB_FIT_RGB 2    /* inputs[1] = U8 [N][H][W][C], the original colour frame */
typedef struct { int N, H, W; int OH, OW; int C; int source; int dtype; int maxval, shift; int siting, range; float kr, kb; } snnhip_rgb_fit_desc;
int snnhip_rgb_fit_plan_create(snnhip_ctx* ctx, const snnhip_rgb_fit_desc* desc, snnhip_plan** out); /* run with snnhip_plan_run_n, 2 inputs */
/* host only, no context: the table of one axis with `in` source samples and `out` outputs: weights [out][4] (capacity >= 4 * out floats) and base
 * [out] ints; output X reads in[clamp(base[X] - 1 + k)] with weights[X][k], k = 0..3.  SNNHIP_SITING_LEFT is the horizontal axis of a left-sited
 * 4:2:0 plane, SNNHIP_SITING_CENTRE everything else.  The plan builds its two tables with this function and keeps them in device memory.
 * SNNHIP_E_INVALID with a message for a ratio outside [1, 8], a null pointer, too little room and an unknown siting. */
int snnhip_rgb_fit_taps(int in, int out, int siting, float* weights, int* base, int capacity);

/* A 4:2:0 video frame in front of an RGB(A) model: the decoder's planes in, the model's NORMALISED INPUT TENSOR at the model's input size out, in one
 * launch -- what lets a classifier, a detector or a style network take NV12 / P010 / I420 / I010 without a CPU conversion.  No RGB frame and no
 * full-resolution float frame exists anywhere (the composition it replaces is yuv_rgb at r = 1, image_u8, resize: three launches, an 8-bit rounding
 * in the middle, 8-bit video only).  DESIGN.md section 4.26.  The contract, stated once:
 *   Shapes: inputs[0] = the luma plane [N][H][W][1]; inputs[1] = the chroma, interleaved CbCr [N][H/2][W/2][2] (snnhip_yuv_tensor_plan_create) or
 *     planar [2N][H/2][W/2][1], plane 2n = Cb and 2n + 1 = Cr of image n (snnhip_yuv_tensor_planar_plan_create, the same desc); both of `src_dtype`,
 *     SNNHIP_U8 or SNNHIP_U16; H and W even.  Output [N][OH][OW][C] of `out_dtype`, SNNHIP_F32 or SNNHIP_F16, C = 3 (R, G, B) or 4 (R, G, B, alpha).
 *     Run with snnhip_plan_run_n, 2 inputs.  Values are float(u >> shift); maxval, shift, siting, range, kr, kb mean what they mean for yuv_rgb.
 *   Source pixel: at luma pixel (Y, X), v_c(Y, X) is yuv_rgb's expression at r = 1 for channel c -- snnhip_bicubic_taps_420(1, siting) along a row,
 *     (1, centre) along a column, what is filtered is the sample minus Coff, horizontal then vertical, the five coefficients of
 *     snnhip_yuv_rgb_coefficients, yl = cy (Y - Yoff), R = yl + crv Cr~, G = yl - (cgv Cr~ + cgu Cb~), B = yl + cbu Cb~, fp32 throughout -- NOT
 *     rounded, and clamped to [0, maxval] as a float.
 *   Sampling: output coordinate o of an axis with `in` source and `out` output samples sits at source position u = (o + 1/2) in / out - 1/2 (resize's
 *     rule; in integers u = ((2o + 1) in - out) / (2 out)).  The positions come from snnhip_yuv_tensor_taps, computed on the host; the kernel does no
 *     position arithmetic.  SNNHIP_YUV_TENSOR_LINEAR: i0 = floor(u), a = the exact fraction u - i0 rounded to double and then to float, source indices
 *     i0 and i0 + 1 clamped to [0, in - 1]; sample_c = top (1 - ay) + bot ay with top = v_c(y0, x0) (1 - ax) + v_c(y0, x1) ax and bot likewise on
 *     row y1, in fp32 (horizontal first, resize's form); two indices that clamp to the same source pixel read the same value.
 *     SNNHIP_YUV_TENSOR_NEAREST: the source pixel floor(((2o + 1) in) / (2 out)) on each axis.  Nothing is low-passed: shrinking aliases as the
 *     reference's bilinear resize does.
 *   Output: t[n][oy][ox][c] = (sample_c - means[c]) * norms[c] for c < 3, t[..][3] = alpha for C = 4; stored as fp32, or rounded to nearest even
 *     as fp16.
 *   Consequences: at OH = H, OW = W every a is 0 and t is the source pixel itself; with means 0 and norms 1, rint(t) is yuv_rgb's value at r = 1
 *     wherever the value is not within yuv_rgb's near-tie eps of a rounding tie.  Neutral chroma gives R = G = B exactly.  In fp32 a value stays within
 *     3.9e-5 / 1.8e-4 / 5.9e-4 (8 / 10 / 12 bits, per unit of |norm|; measured, tests/yuv_tensor_ref.py) of a float64 evaluation; the tests hold
 *     every output element to |norms[c]| E, E = four times that: 1.56e-4 / 7.2e-4 / 2.36e-3, plus half an fp16 ulp for fp16 output.
 * Plan creation returns SNNHIP_E_INVALID with a message starting "yuv_tensor desc" for everything yuv_rgb refuses (dtype, maxval, shift, maxval + 1
 * not a multiple of 256, siting, range, kr / kb), bad dims, an odd H or W, OH or OW below 1, C outside {3, 4}, an unknown filter and an out_dtype that
 * is neither SNNHIP_F32 nor SNNHIP_F16.  snnhip_plan_run_n refuses, with a message starting "yuv_tensor" / "yuv_tensor_planar", a tensor of another
 * dtype or shape at any position.  snnhip_plan_describe: "yuv_tensor_u8 c=4 f32 linear siting=left range=limited 1080x1920->224x224 tile=256
 * taps=bilinear ... kernel=yuv_tensor_kernel" (the tile in flat output pixels per block; taps=single when one source pixel serves an output pixel:
 * nearest, or linear tables whose weights are all 0, ratio 1 among them).  snnhip_plan_cost counts both inputs once and the output once.
 * Not offered: anti-aliased shrinking (the reference's resize is a plain bilinear sampler, and plane_fit's stretched cubic stops at 1/2);
 * letterboxing and crop rectangles; 4:2:2 / 4:4:4; BGR order; video in front of the luma-only model paths, which have their own plans above. */
#define SNNHIP_YUV_TENSOR_NEAREST 0
#define SNNHIP_YUV_TENSOR_LINEAR 1
typedef struct { int N, H, W; int OH, OW, C; int src_dtype, out_dtype; int maxval, shift; int siting, range; float kr, kb; int filter; float means[3], norms[3]; float alpha; } snnhip_yuv_tensor_desc; /* H, W: the LUMA plane */
int snnhip_yuv_tensor_plan_create(snnhip_ctx* ctx, const snnhip_yuv_tensor_desc* desc, snnhip_plan** out);        /* run with snnhip_plan_run_n, 2 inputs */
int snnhip_yuv_tensor_planar_plan_create(snnhip_ctx* ctx, const snnhip_yuv_tensor_desc* desc, snnhip_plan** out); /* run with snnhip_plan_run_n, 2 inputs */
/* host only, no context: the table of one axis with `in` source samples and `out` outputs: weight [out] floats (a; 0 for nearest) and index [out][2]
 * ints (i0 and i0 + 1 clamped to the axis; nearest: the source index twice); `capacity` is the room in coordinates (weight holds that many floats,
 * index twice as many ints).  The plan builds its two tables with this function and keeps them in device memory.  SNNHIP_E_INVALID with a message
 * for a null pointer, in or out outside 1 .. 2^30, an unknown filter and too little room. */
int snnhip_yuv_tensor_taps(int in, int out, int filter, float* weight, int* index, int capacity);

/* The output tensor of an RGB(A) model to the planes of a 4:2:0 video frame of the same extent, in one launch: what a hardware or software encoder
 * takes (NV12 / P010 / I420 / I010) behind a style or enhancement network, 1.5 bytes per pixel (3 for 10-bit) instead of a float tensor or a packed
 * RGB8 frame crossing the host link.  It is the other end of yuv_tensor, and the decimation filter that rgb_cbcr's r = 1 lacks.  DESIGN.md section
 * 4.27.  The contract, stated once:
 *   Shapes: inputs[0] = the tensor [N][H][W][C] of `in_dtype`, SNNHIP_F32 or SNNHIP_F16, C = 3 (R, G, B) or 4 (channel 3 is ignored, whatever it holds);
 *     H and W even, at least 2.  outputs[0] = the luma plane [N][H][W][1]; outputs[1] = the chroma, interleaved CbCr [N][H/2][W/2][2]
 *     (snnhip_tensor_yuv_plan_create) or planar [2N][H/2][W/2][1], plane 2n = Cb and 2n + 1 = Cr of image n (snnhip_tensor_yuv_planar_plan_create, the
 *     same desc); both of `out_dtype`, SNNHIP_U8 or SNNHIP_U16.  maxval, shift, siting, range, kr, kb mean what they mean for yuv_rgb.  The plan has
 *     two outputs: run it with snnhip_plan_run_io, 1 input, 2 outputs.
 *   Pixel: p_c = clamp(fmaf(x_c, scale[c], offset[c]), 0, maxval) in fp32 (an fp16 tensor's values widened): full-range RGB in units of the output
 *     depth.  A model that emits 0..255 uses scale 1 for 8-bit and 1023 / 255 for 10-bit; a tanh model maxval / 2 for both scale and offset.
 *   Luma: ylo = kr R + kg G + kb B in fp32, unquantised (the one device function of rgb_luma, ycc_merge and rgb_cbcr, kg = 1 - kr - kb as there);
 *     with k = (maxval + 1) / 256 and Yoff, Yrange, Coff, Crange of yuv_rgb's matrix for the range, ys = Yrange / maxval, Y = Yoff + ys ylo,
 *     q = unsigned(clamp(rint(Y), 0, maxval)) << shift, ties to even.
 *   Chroma differences, per luma pixel: dB = B - ylo, dR = R - ylo, unquantised.
 *   Decimation: chroma sample (J, I) reads luma rows 2J and 2J + 1 with weights 1/2, 1/2 (the vertical axis is always centred, as everywhere in this
 *     family).  Along a row SNNHIP_SITING_CENTRE reads columns 2I and 2I + 1 with weights 1/2, 1/2; SNNHIP_SITING_LEFT reads columns 2I - 1, 2I, 2I + 1
 *     with weights 1/4, 1/2, 1/4, the index clamped to [0, W - 1] (only column -1 can clamp: W is even).  Horizontal first, then vertical, in fp32, in
 *     the order (w0 d0 + w1 d1) + w2 d2.  The weights are exact in binary: there is no table.
 *   Chroma matrix: cbs = Crange / (2 (1 - kb) maxval), crs = Crange / (2 (1 - kr) maxval), computed in double and rounded to float: the reciprocals of
 *     yuv_rgb's cbu and crv.  Cb = Coff + cbs dB~, Cr = Coff + crs dR~, through the same quantiser.
 *   Consequences: a grey tensor (R = G = B after the map) gives Cb = Cr = Coff in every sample; a constant tensor gives constant planes; on a 2 x 2-
 *     replicated tensor both sitings agree except in column 0.  In fp32 the value in front of the rounding stays within 3.1e-5 / 1.25e-4 / 4.8e-4
 *     (8 / 10 / 12 bits; measured, tests/tensor_yuv_ref.py) of a float64 evaluation.
 * Plan creation returns SNNHIP_E_INVALID with a message starting "tensor_yuv desc" for everything yuv_rgb refuses (dtype of the planes, maxval, shift,
 * maxval + 1 not a multiple of 256, siting, range, kr / kb), C outside {3, 4}, an odd or non-positive H or W, N < 1 and an in_dtype that is neither
 * SNNHIP_F32 nor SNNHIP_F16.  snnhip_plan_run and snnhip_plan_run_n refuse this plan with a message starting "tensor_yuv"; snnhip_plan_run_io refuses,
 * with a message, a wrong n_in or n_out and a tensor of another dtype or shape at any position.  snnhip_plan_describe: "tensor_yuv_u8 c=3 f16
 * siting=left range=limited 720x1280 tile=2048 ... kernel=tensor_yuv_kernel" (tensor_yuv_planar_... / tensor_yuv_planar_kernel for planar chroma; the
 * tile in luma pixels per block).  snnhip_plan_cost counts the input once and both outputs once.
 * Not offered: resizing at this end (a fitted encoder size is plane_fit behind it); 4:2:2 / 4:4:4; BGR order; a cubic or longer decimation filter;
 * folding the conversion into a model's last convolution. */
typedef struct { int N, H, W, C; int in_dtype, out_dtype; int maxval, shift; int siting, range; float kr, kb; float scale[3], offset[3]; } snnhip_tensor_yuv_desc;
int snnhip_tensor_yuv_plan_create(snnhip_ctx* ctx, const snnhip_tensor_yuv_desc* desc, snnhip_plan** out);        /* chroma out: [N][H/2][W/2][2], interleaved CbCr (NV12 / P010) */
int snnhip_tensor_yuv_planar_plan_create(snnhip_ctx* ctx, const snnhip_tensor_yuv_desc* desc, snnhip_plan** out); /* chroma out: [2N][H/2][W/2][1], plane 2n = Cb, 2n + 1 = Cr (I420 / I010) */
/* host only, no context: out[0..4] = Yoff, ys, Coff, cbs, crs of the map above (capacity >= 5 floats) */
int snnhip_tensor_yuv_coefficients(int maxval, int range, float kr, float kb, float* out, int capacity);

/* Frame quality on the device: PSNR and SSIM between a test frame and a reference frame, so that what an arithmetic choice (fused fp32, the fp16
 * opt-in, 8 / 10 / 12-bit frame ends) or a trained model costs in picture quality can be stated in dB without downloading every output frame.
 * DESIGN.md section 4.22.  The reference ships a host-side comparison script only (tools/misc/imageComparison.py).  The definition, stated once
 * (tests/metrics_ref.py restates it in NumPy):
 *   Shapes: inputs[0] = the test frame a, inputs[1] = the reference frame b, both [N][H][W][C] of the desc's dtype, SNNHIP_U8 or SNNHIP_U16, C = 1..4
 *     interleaved; run with snnhip_plan_run_n, 2 inputs.  The sample value is v = u >> shift (shift = 0 for SNNHIP_U8): the bits below `shift` are
 *     ignored, exactly as u16_in ignores them.  Results are per image n and channel c; images and channels never mix.
 *   SSE and PSNR: sse = sum (a - b)^2 over all H * W pixels, an exact unsigned 64-bit integer; pixels = H * W;
 *     psnr_db = 10 log10(maxval^2 pixels / sse) in double, +inf for sse == 0.
 *   SSIM: the integer-moment form on 8x8 windows with a 4-pixel step, modelled on what x264 and ffmpeg's ssim filter compute.  bh = H >> 2,
 *     bw = W >> 2; rows and columns past 4 bh, 4 bw take no part in SSIM (they do in SSE).  Every 4x4 block has the exact integers s1 = sum a,
 *     s2 = sum b, ss = sum (a^2 + b^2), s12 = sum a b.  A window is the sum of a 2x2 group of neighbouring blocks: (bh - 1)(bw - 1) windows.  Per
 *     window, from the integer moments converted to double (all below 2^53 up to 16 bits):
 *         c1 = 0.01^2 maxval^2 64,  c2 = 0.03^2 maxval^2 64 63,  vars = 64 ss - s1^2 - s2^2,  covar = 64 s12 - s1 s2,
 *         t = (2 s1 s2 + c1)(2 covar + c2) / ((s1^2 + s2^2 + c1)(vars + c2))
 *     ssim = sum t / windows, in double.  Equal frames give t = 1 exactly in every window, hence ssim = 1.0 exactly.
 *   Output: SNNHIP_F32 [N][1][C][2] = {psnr_db, ssim}, the doubles rounded to float (psnr_db may be +inf).  The exact results stay in the plan:
 *     snnhip_frame_metrics_read waits for the context's stream, copies the N * C rows (n-major) {sse, pixels, windows, ssim_sum} to the host and
 *     returns their count (a negative SNNHIP_E_* code on failure; max_rows below N * C is SNNHIP_E_INVALID).  snnhip_frame_metrics_psnr is the dB
 *     formula on the host, device-free, for callers that add sse over frames.
 *   Two launches, no atomics, no memset: a tile kernel that leaves one partial per (block, channel) in a scratch buffer of the plan and a fold kernel
 *     that adds them in index order.  A result is bit-identical from run to run and the plan can be recorded in an snnhip_graph.
 * Plan creation returns SNNHIP_E_INVALID with a message starting "frame_metrics" for C outside 1..4, a dtype that is neither SNNHIP_U8 nor SNNHIP_U16,
 * H or W below 8 (no window would exist) and a maxval / shift that does not fit the container (shift 0 for 8-bit frames, 0..15 for 16-bit ones,
 * 1 <= maxval, maxval << shift within the container: chroma_up's rules, but up to maxval 65535 with shift 0, integers have no rounding contract to
 * keep); snnhip_plan_run_n for a tensor of another dtype or shape at either input and an output that is not SNNHIP_F32 [N][1][C][2].
 * snnhip_plan_describe: "frame_metrics_u8 c=1 tile=32x128 ... kernel=frame_metrics_tile_kernel+frame_metrics_fold_kernel".  snnhip_plan_cost counts
 * both frames once plus the partials, written and read. */
typedef struct { int N, H, W, C; int dtype; int maxval, shift; } snnhip_frame_metrics_desc;
int snnhip_frame_metrics_plan_create(snnhip_ctx* ctx, const snnhip_frame_metrics_desc* desc, snnhip_plan** out); /* run with snnhip_plan_run_n, 2 inputs */
typedef struct { unsigned long long sse, pixels, windows; double ssim_sum; } snnhip_frame_metrics_row;
int snnhip_frame_metrics_read(snnhip_plan* plan, snnhip_frame_metrics_row* rows, int max_rows);
double snnhip_frame_metrics_psnr(unsigned long long sse, unsigned long long pixels, int maxval);
/* index of the largest element of image n of t (first one on ties, like std::max_element in MixedInferenceCore::run, core.cpp:228-234,
 * which reports index + 1 as classifierOutput); stream sync + a 4-byte D2H */
int snnhip_tensor_argmax(const snnhip_tensor* t, int n, int* out_index);

/* Try to replace a linear chain of plans (plan[i+1] consumes only plan[i]'s output) by fused kernels.
 * On success *out runs the whole chain in <= n launches; intermediate tensors that become internal are never
 * materialised.  Returns SNNHIP_E_UNSUPPORTED when no fusion rule matches (callers keep the unfused plans).
 * Implemented rule set: see DESIGN.md section 4 (ESPCN: conv5x5(1->16)+conv3x3(16->16), conv3x3(16->4)+subpixel). */
int snnhip_chain_plan_create(snnhip_ctx* ctx, snnhip_plan* const* plans, int n, snnhip_plan** out);
/* The fp16 ESPCN rules (SNNHIP_ESPCN_F16=1) keep their weights as lane-ordered fp16 images for the f16 matrix cores.  This
 * is the packing itself, host side only (no context, no device), so that it can be checked without a GPU.  w_oihw is fp32 and is rounded to nearest
 * even; out receives the halfs' bit patterns, *count how many.
 *   ic = 1, k = 3 or 5:        [16][1][k][k] -> 512 halfs,   out[lane*8 + j] = W[oc = lane%16][tap = 8*(lane/16) + j], zero from tap k*k on
 *   ic = 16, k = 3, r = 0:     [16][16][3][3] -> 2304 halfs, MFMA row = output channel
 *   ic = 16, k = 3, r = 2,3,4: [r*r][16][3][3] -> 2304 halfs, MFMA row 4*dy + dx = channel r*dy + dx (other rows zero)
 *       out[(s*64 + lane)*8 + j] = W[row lane%16][ic = 8*(g%2) + j][tap = 2*s + g/2],  s = 0..3, g = lane/16, j = 0..7
 *       out[2048 + lane*4 + j]   = W[row lane%16][ic = 4*g + j][tap = 8],               j = 0..3 */
int snnhip_espcn_f16_pack_weights(const float* w_oihw, int ic, int k, int r, unsigned short* out, int capacity, int* count);
/* The same for the rules at the published ESPCN widths, 1 -> 64 -> 32 -> r*r (espcn_f16_wide.hip): every K-step of a 3x3
 * image is one tap and 32 input channels of v_mfma_f32_16x16x32_f16, MFMA rows in blocks of 16.  Host side only; any other shape returns
 * SNNHIP_E_INVALID.
 *   oc = 64, ic = 1, k = 3 or 5, r = 0:   [64][1][k][k] -> 2048 halfs,   out[(mb*64 + lane)*8 + j] = W[oc = 16*mb + lane%16][tap = 8*(lane/16) + j],
 *                                                                         zero from tap k*k on
 *   oc = 32, ic = 64, k = 3, r = 0:       [32][64][3][3] -> 18432 halfs, MFMA row = output channel, MB = 2 row blocks, KC = 2 K-steps per tap
 *   oc = r*r, ic = 32, k = 3, r = 2,3,4:  [r*r][32][3][3] -> 4608 halfs, MFMA row 4*dy + dx = channel r*dy + dx (other rows zero), MB = 1, KC = 1
 *       out[((ks*MB + mb)*64 + lane)*8 + j] = W[row 16*mb + lane%16][ic = 32*(ks % KC) + 8*(lane/16) + j][tap = ks / KC],  ks = 0 .. 9*KC - 1, j = 0..7 */
int snnhip_espcn_f16_wide_pack_weights(const float* w_oihw, int oc, int ic, int k, int r, unsigned short* out, int capacity, int* count);

/* Graph-level fusion: the ONE place where an operator DAG is searched for fusable groups (the host mirror's
 * HipBackend::finalizeStages and the Python GraphRunner both call it; the rules themselves are snnhip_chain_plan_create's).
 * nodes[i] describes operator i in execution order: its per-layer plan (NULL = opaque operator that never fuses: a CPU stage, a
 * multi-pass layer), its producers (node index, or -(k+1) for model input k) and whether its tensor must exist (model output, dump).
 * out[i] says what to run instead: plan == NULL -> node i's work moved into a later node's plan and its tensor is never produced;
 * owned == 0 -> the node's own plan (run it with out[i].inputs: a folded identity producer, e.g. a Flatten in front of a Dense layer, is
 * skipped by re-wiring); owned == 1 -> a new fused plan the caller destroys with
 * snnhip_plan_destroy, to be run with out[i].inputs (it produces node i's tensor).  The per-layer plans must outlive the fused ones.
 * Groups searched: Conv2D -> Add where the Add is the convolution's only consumer (rule E, two-input fused plan), and maximal
 * linear runs (each operator the sole consumer of the previous one) handed to the chain planner (rules A-D, F). */
#define SNNHIP_GRAPH_MAX_INPUTS 4
typedef struct snnhip_graph_node {
    snnhip_plan* plan;
    int n_inputs;
    int inputs[SNNHIP_GRAPH_MAX_INPUTS];
    int keep;
} snnhip_graph_node;
typedef struct snnhip_fused_node {
    snnhip_plan* plan;
    int owned;
    int n_inputs;
    int inputs[SNNHIP_GRAPH_MAX_INPUTS];
} snnhip_fused_node;
int snnhip_graph_fuse(snnhip_ctx* ctx, const snnhip_graph_node* nodes, int n, snnhip_fused_node* out);

int snnhip_plan_run(snnhip_plan* plan, const snnhip_tensor* in, snnhip_tensor* out);
/* multi-input ops (add, concat): inputs[n_in] */
int snnhip_plan_run_n(snnhip_plan* plan, const snnhip_tensor* const* inputs, int n_in, snnhip_tensor* out);
/* a plan with more than one output: the tensor_yuv plans (1 input; outputs[0] = the luma plane, outputs[1] = the chroma).  Every other plan is
 * refused with a message; the two functions above refuse a tensor_yuv plan.  The same launch trace, guard mode and graph capture as those two. */
int snnhip_plan_run_io(snnhip_plan* plan, const snnhip_tensor* const* inputs, int n_in, snnhip_tensor* const* outputs, int n_out);
int snnhip_plan_output_dims(const snnhip_plan* plan, int dims_nhwc[4]);
/* Human-readable kernel-variant description ("conv2d_mfma_f32 tile=...") for logs and tests. */
int snnhip_plan_describe(const snnhip_plan* plan, char* buf, size_t buflen);
/* Algorithmic work of one run: flops and true-channel HBM bytes (inputs once + outputs once + weights once). */
int snnhip_plan_cost(const snnhip_plan* plan, double* flops, double* bytes);
int snnhip_plan_destroy(snnhip_plan* plan);

/* A plan executes as one or more kernel launches ("steps": 1 for plain operators, one per fused kernel for chains).
 * With profiling enabled every launch is bracketed by a hipEvent pair on the context stream (the analogue of the
 * reference's per-stage DeviceTimer, core/src/ic2/core.cpp:140-153).  snnhip_plan_profile_read waits for the
 * recorded events, returns the summed duration and launch count of step `step` since the last read, and resets. */
int snnhip_plan_num_steps(const snnhip_plan* plan);
int snnhip_plan_step_describe(const snnhip_plan* plan, int step, char* buf, size_t buflen);
int snnhip_plan_step_cost(const snnhip_plan* plan, int step, double* flops, double* bytes);
int snnhip_plan_profile_enable(snnhip_plan* plan, int enable);
int snnhip_plan_profile_read(snnhip_plan* plan, int step, double* total_ms, int* launches);

/* ---- launch trace: per-KERNEL-FUNCTION timing of everything the library launches (measurement only) -------------------------
 * The reference times per STAGE (DeviceTimer around a render pass, core/src/ic2/core.cpp:140-153,392-404); a fused plan or a split-K
 * convolution is several launches per stage, and a roofline is a statement about ONE kernel.  Between snnhip_trace_begin and
 * snnhip_trace_end every kernel launch of the process's plans is issued with its own event pair (the dispatch packet's start / end
 * stamps: the durations rocprofv3 --kernel-trace reports) and booked on the plan that launched it; plans must be RUN, not replayed
 * from a captured graph, while a trace is on.  snnhip_trace_report writes JSON: launches grouped by kernel function (template
 * instantiations listed inside), each with launch count, summed duration, and the algorithmic flops / HBM bytes of the plan
 * invocations whose longest launch it was (a plan's cost = snnhip_plan_cost's flops and, for a fused plan, what the fused launch
 * itself has to move instead of the per-layer sum).  *needed = bytes the full report takes (call with buf == NULL to size it). */
int snnhip_trace_begin(void);
int snnhip_trace_end(void);
int snnhip_trace_report(char* buf, size_t buflen, size_t* needed);

/* ---- device timers (hipEvent pairs on the context stream) ---------------------------------------- */

int snnhip_timer_create(snnhip_ctx* ctx, snnhip_timer** out);
int snnhip_timer_start(snnhip_timer* t);
int snnhip_timer_stop(snnhip_timer* t);
int snnhip_timer_elapsed_ms(snnhip_timer* t, float* ms); /* waits for the stop event */
int snnhip_timer_destroy(snnhip_timer* t);

/* ---- launch graphs ------------------------------------------------------------------------------------
 * The reference records one command buffer per inference and replays it (vulkanBackend.cpp:80-106: prepareRun records, sync submits).
 * The HIP counterpart is a captured hipGraph: every snnhip_plan_run* between begin and end is recorded instead of executed (plans must
 * be run with the same tensors they will be replayed on; profiling must be off), and snnhip_graph_launch replays the whole sequence with
 * one host call -- what a 65-kernel MobileNetV2 or a 54-kernel Candy inference needs to stop being launch-bound. */
typedef struct snnhip_graph snnhip_graph;
int snnhip_graph_begin_capture(snnhip_ctx* ctx);
int snnhip_graph_end_capture(snnhip_ctx* ctx, snnhip_graph** out);
int snnhip_graph_launch(snnhip_graph* g); /* enqueues on the context stream */
int snnhip_graph_num_nodes(const snnhip_graph* g);
int snnhip_graph_destroy(snnhip_graph* g);

#ifdef __cplusplus
}
#endif
#endif
