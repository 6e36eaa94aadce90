// frame_u8.hip -- 8-bit frames at both ends of a model (include/snnhip.h: snnhip_u8_in_plan_create / snnhip_u8_out_plan_create).
//
//   u8_in :  U8 [P][C] -> T [P][C],   y = (float(u) - means[c]) * norms[c]
//   u8_out:  T [P][C] -> U8 [P][C],   q = clamp(rint(fmaf(x, scale[c], offset[c])), 0, 255), NaN -> 0
// (P = N*H*W pixels, C = 1..4, T = float or _Float16.)  The reference normalises on the host or in a resize pass (image.cpp:712-796,
// ImageTexture::convertToRGBA32FAndNormalize) and reads results back as floats; ColorFormat::R8 / RGB8 / RGBA8 (color.h) name these formats.
// Both are HBM-bound streams: one lane takes 4 pixels = 4C bytes (C dwords) and 4C elements (C 16-byte fp32 or 8-byte fp16 accesses), grid-stride;
// the last P % 4 pixels take a scalar tail.  Chain rules A8 / B8 (chain_fuse.hip) compute the same two expressions inside the ESPCN kernels.
#include "epilogue.h"
#include "plan_util.h"
#include "snnhip_internal.h"

namespace snnhip {
namespace {

struct U8Affine {
    float a[4], b[4]; // u8_in: means, norms; u8_out: scale, offset
};

template <int C, typename T>
__global__ __launch_bounds__(256) void u8_in_kernel(size_t pixels, U8Affine f, const unsigned char* __restrict__ x, T* __restrict__ y) {
    const size_t groups = pixels / 4;
    const size_t stride = static_cast<size_t>(gridDim.x) * 256;
    for (size_t g = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; g < groups; g += stride) {
        unsigned w[C];
#pragma unroll
        for (int k = 0; k < C; ++k) w[k] = reinterpret_cast<const unsigned*>(x + g * 4 * C)[k];
        float v[4 * C];
#pragma unroll
        for (int e = 0; e < 4 * C; ++e) v[e] = (static_cast<float>((w[e >> 2] >> (8 * (e & 3))) & 255u) - f.a[e % C]) * f.b[e % C];
#pragma unroll
        for (int k = 0; k < C; ++k) {
            float q[4] = {v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]};
            stv<T, 4>(y + (g * 4 * C + 4 * k), q);
        }
    }
    for (size_t i = groups * 4 * C + static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < pixels * C; i += stride) {
        const int c = static_cast<int>(i % C);
        float q[1] = {(static_cast<float>(x[i]) - f.a[c]) * f.b[c]};
        stv<T, 1>(y + i, q);
    }
}

template <int C, typename T>
__global__ __launch_bounds__(256) void u8_out_kernel(size_t pixels, U8Affine f, const T* __restrict__ x, unsigned char* __restrict__ y) {
    const size_t groups = pixels / 4;
    const size_t stride = static_cast<size_t>(gridDim.x) * 256;
    for (size_t g = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; g < groups; g += stride) {
        float v[4 * C];
#pragma unroll
        for (int k = 0; k < C; ++k) {
            float q[4];
            ldv<T, 4>(x + (g * 4 * C + 4 * k), q);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * k + j] = q[j];
        }
        unsigned w[C];
#pragma unroll
        for (int k = 0; k < C; ++k) w[k] = 0u;
#pragma unroll
        for (int e = 0; e < 4 * C; ++e) w[e >> 2] |= quantize_u8(v[e], f.a[e % C], f.b[e % C]) << (8 * (e & 3));
#pragma unroll
        for (int k = 0; k < C; ++k) reinterpret_cast<unsigned*>(y + g * 4 * C)[k] = w[k];
    }
    for (size_t i = groups * 4 * C + static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < pixels * C; i += stride) {
        const int c = static_cast<int>(i % C);
        float q[1];
        ldv<T, 1>(x + i, q);
        y[i] = static_cast<unsigned char>(quantize_u8(q[0], f.a[c], f.b[c]));
    }
}

const char* dtype_name(int dt) { return dt == SNNHIP_F16 ? "f16" : "f32"; }

struct U8InPlan : snnhip_plan {
    snnhip_u8_in_desc d;
    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        SNNHIP_REQUIRE(nIn == 1, "u8_in: expects 1 input, got %d", nIn);
        SNNHIP_REQUIRE(in[0]->dtype == SNNHIP_U8, "u8_in: the input tensor must be SNNHIP_U8, got dtype %d", in[0]->dtype);
        SNNHIP_REQUIRE(out->dtype == d.dtype, "u8_in: output dtype %d, the plan was built for %d", out->dtype, d.dtype);
        SNNHIP_REQUIRE(dims_match(in[0], d.N, d.H, d.W, d.C) && dims_match(out, d.N, d.H, d.W, d.C), "u8_in: tensor dims do not match the plan");
        const size_t pixels = static_cast<size_t>(d.N) * d.H * d.W;
        U8Affine f;
        for (int c = 0; c < 4; ++c) {
            f.a[c] = d.means[c];
            f.b[c] = d.norms[c];
        }
        const unsigned g = grid_for(ctx, pixels / 4 + 1);
        const unsigned char* src = reinterpret_cast<const unsigned char*>(in[0]->data);
#define SNNHIP_U8_IN(CC) SNNHIP_LAUNCH((u8_in_kernel<CC, T>), dim3(g), dim3(256), 0, ctx->stream, pixels, f, src, mptr<T>(out))
        SNNHIP_WITH_T(out->dtype, if (d.C == 1) SNNHIP_U8_IN(1); else if (d.C == 2) SNNHIP_U8_IN(2); else if (d.C == 3) SNNHIP_U8_IN(3); else SNNHIP_U8_IN(4););
#undef SNNHIP_U8_IN
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }
};

struct U8OutPlan : snnhip_plan {
    snnhip_u8_out_desc d;
    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        SNNHIP_REQUIRE(nIn == 1, "u8_out: expects 1 input, got %d", nIn);
        SNNHIP_REQUIRE(in[0]->dtype == d.dtype, "u8_out: input dtype %d, the plan was built for %d", in[0]->dtype, d.dtype);
        SNNHIP_REQUIRE(out->dtype == SNNHIP_U8, "u8_out: the output tensor must be SNNHIP_U8, got dtype %d", out->dtype);
        SNNHIP_REQUIRE(dims_match(in[0], d.N, d.H, d.W, d.C) && dims_match(out, d.N, d.H, d.W, d.C), "u8_out: tensor dims do not match the plan");
        const size_t pixels = static_cast<size_t>(d.N) * d.H * d.W;
        U8Affine f;
        for (int c = 0; c < 4; ++c) {
            f.a[c] = d.scale[c];
            f.b[c] = d.offset[c];
        }
        const unsigned g = grid_for(ctx, pixels / 4 + 1);
        unsigned char* dst = reinterpret_cast<unsigned char*>(out->data);
#define SNNHIP_U8_OUT(CC) SNNHIP_LAUNCH((u8_out_kernel<CC, T>), dim3(g), dim3(256), 0, ctx->stream, pixels, f, cptr<T>(in[0]), dst)
        SNNHIP_WITH_T(in[0]->dtype, if (d.C == 1) SNNHIP_U8_OUT(1); else if (d.C == 2) SNNHIP_U8_OUT(2); else if (d.C == 3) SNNHIP_U8_OUT(3); else SNNHIP_U8_OUT(4););
#undef SNNHIP_U8_OUT
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }
};

} // namespace

bool u8_in_plan_desc(const snnhip_plan* plan, snnhip_u8_in_desc* d) {
    auto* p = dynamic_cast<const U8InPlan*>(plan);
    if (p && d) *d = p->d;
    return p != nullptr;
}

bool u8_out_plan_desc(const snnhip_plan* plan, snnhip_u8_out_desc* d) {
    auto* p = dynamic_cast<const U8OutPlan*>(plan);
    if (p && d) *d = p->d;
    return p != nullptr;
}

} // namespace snnhip

using namespace snnhip;

extern "C" {

int snnhip_u8_in_plan_create(snnhip_ctx* ctx, const snnhip_u8_in_desc* desc, snnhip_plan** out) {
    SNNHIP_REQUIRE(ctx && desc && out, "u8_in_plan_create: null argument");
    SNNHIP_REQUIRE(desc->N > 0 && desc->H > 0 && desc->W > 0, "u8_in desc: bad dims %dx%dx%d", desc->N, desc->H, desc->W);
    SNNHIP_REQUIRE(desc->C >= 1 && desc->C <= 4, "u8_in desc: %d channels (1..4: R8, RG8, RGB8, RGBA8)", desc->C);
    SNNHIP_REQUIRE(desc->dtype == SNNHIP_F32 || desc->dtype == SNNHIP_F16, "u8_in desc: dtype %d (SNNHIP_F32 or SNNHIP_F16)", desc->dtype);
    auto* plan = new U8InPlan();
    plan->ctx = ctx;
    plan->dtype = desc->dtype;
    plan->rawInput = SNNHIP_U8;
    plan->d = *desc;
    for (int i = 0; i < 4; ++i) {
        plan->inDims[i] = plan->outDims[i] = (&desc->N)[i];
    }
    const double elems = static_cast<double>(desc->N) * desc->H * desc->W * desc->C;
    plan->bytes = elems * (1 + (desc->dtype == SNNHIP_F16 ? 2 : 4));
    char buf[128];
    snprintf(buf, sizeof(buf), "u8_in_%s c=%d %dx%d kernel=u8_in_kernel", dtype_name(desc->dtype), desc->C, desc->H, desc->W);
    plan->desc = buf;
    *out = plan;
    return SNNHIP_OK;
}

int snnhip_u8_out_plan_create(snnhip_ctx* ctx, const snnhip_u8_out_desc* desc, snnhip_plan** out) {
    SNNHIP_REQUIRE(ctx && desc && out, "u8_out_plan_create: null argument");
    SNNHIP_REQUIRE(desc->N > 0 && desc->H > 0 && desc->W > 0, "u8_out desc: bad dims %dx%dx%d", desc->N, desc->H, desc->W);
    SNNHIP_REQUIRE(desc->C >= 1 && desc->C <= 4, "u8_out desc: %d channels (1..4: R8, RG8, RGB8, RGBA8)", desc->C);
    SNNHIP_REQUIRE(desc->dtype == SNNHIP_F32 || desc->dtype == SNNHIP_F16, "u8_out desc: dtype %d (SNNHIP_F32 or SNNHIP_F16)", desc->dtype);
    auto* plan = new U8OutPlan();
    plan->ctx = ctx;
    plan->dtype = desc->dtype;
    plan->rawOutput = SNNHIP_U8;
    plan->d = *desc;
    for (int i = 0; i < 4; ++i) {
        plan->inDims[i] = plan->outDims[i] = (&desc->N)[i];
    }
    const double elems = static_cast<double>(desc->N) * desc->H * desc->W * desc->C;
    plan->bytes = elems * (1 + (desc->dtype == SNNHIP_F16 ? 2 : 4));
    char buf[128];
    snprintf(buf, sizeof(buf), "u8_out_%s c=%d %dx%d kernel=u8_out_kernel", dtype_name(desc->dtype), desc->C, desc->H, desc->W);
    plan->desc = buf;
    *out = plan;
    return SNNHIP_OK;
}

} // extern "C"
