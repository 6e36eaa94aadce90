// frame_u16.hip -- 16-bit frames (10 / 12 / 16-bit video in 2-byte containers) at both ends of a model (include/snnhip.h:
// snnhip_u16_in_plan_create / snnhip_u16_out_plan_create).
//
//   u16_in :  U16 [P][C] -> T [P][C],   y = (float(u >> shift) - means[c]) * norms[c]
//   u16_out:  T [P][C] -> U16 [P][C],   q = unsigned(clamp(rint(fmaf(x, scale[c], offset[c])), 0, maxval)) << shift, NaN -> 0
// (P = N*H*W pixels, C = 1..4, T = float or _Float16.)  `shift` and `maxval` name the container layout: low-aligned 10 / 12-bit (maxval 1023 / 4095,
// shift 0), P010-style high-aligned 10-bit (maxval 1023, shift 6), full 16-bit (maxval 65535).  ColorFormat::R16 / RGB16 / RGBA16 are these formats.
// Same shape as frame_u8.hip's streams: one lane takes 4 pixels = 8C bytes of frame (2C dwords) and 4C elements (C 16-byte fp32 or 8-byte fp16
// accesses), grid-stride; the last P % 4 pixels take a scalar tail.
#include "epilogue.h"
#include "plan_util.h"
#include "snnhip_internal.h"

namespace snnhip {
namespace {

struct U16Affine {
    float a[4], b[4]; // u16_in: means, norms; u16_out: scale, offset
    float maxval;     // u16_out only
    int shift;
};

template <int C, typename T>
__global__ __launch_bounds__(256) void u16_in_kernel(size_t pixels, U16Affine f, const unsigned short* __restrict__ x, T* __restrict__ y) {
    const size_t groups = pixels / 4;
    const size_t stride = static_cast<size_t>(gridDim.x) * 256;
    for (size_t g = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; g < groups; g += stride) {
        unsigned w[2 * C];
#pragma unroll
        for (int k = 0; k < 2 * C; ++k) w[k] = reinterpret_cast<const unsigned*>(x + g * 4 * C)[k];
        float v[4 * C];
#pragma unroll
        for (int e = 0; e < 4 * C; ++e) v[e] = (static_cast<float>(((w[e >> 1] >> (16 * (e & 1))) & 65535u) >> f.shift) - f.a[e % C]) * f.b[e % C];
#pragma unroll
        for (int k = 0; k < C; ++k) {
            float q[4] = {v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]};
            stv<T, 4>(y + (g * 4 * C + 4 * k), q);
        }
    }
    for (size_t i = groups * 4 * C + static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < pixels * C; i += stride) {
        const int c = static_cast<int>(i % C);
        float q[1] = {(static_cast<float>(static_cast<unsigned>(x[i]) >> f.shift) - f.a[c]) * f.b[c]};
        stv<T, 1>(y + i, q);
    }
}

template <int C, typename T>
__global__ __launch_bounds__(256) void u16_out_kernel(size_t pixels, U16Affine f, const T* __restrict__ x, unsigned short* __restrict__ y) {
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
        unsigned w[2 * C];
#pragma unroll
        for (int k = 0; k < 2 * C; ++k) w[k] = 0u;
#pragma unroll
        for (int e = 0; e < 4 * C; ++e) w[e >> 1] |= (quantize_u16(v[e], f.a[e % C], f.b[e % C], f.maxval) << f.shift) << (16 * (e & 1));
#pragma unroll
        for (int k = 0; k < 2 * C; ++k) reinterpret_cast<unsigned*>(y + g * 4 * C)[k] = w[k];
    }
    for (size_t i = groups * 4 * C + static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < pixels * C; i += stride) {
        const int c = static_cast<int>(i % C);
        float q[1];
        ldv<T, 1>(x + i, q);
        y[i] = static_cast<unsigned short>(quantize_u16(q[0], f.a[c], f.b[c], f.maxval) << f.shift);
    }
}

const char* dtype_name(int dt) { return dt == SNNHIP_F16 ? "f16" : "f32"; }

struct U16InPlan : snnhip_plan {
    snnhip_u16_in_desc d;
    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        SNNHIP_REQUIRE(nIn == 1, "u16_in: expects 1 input, got %d", nIn);
        SNNHIP_REQUIRE(in[0]->dtype == SNNHIP_U16, "u16_in: the input tensor must be SNNHIP_U16, got dtype %d", in[0]->dtype);
        SNNHIP_REQUIRE(out->dtype == d.dtype, "u16_in: output dtype %d, the plan was built for %d", out->dtype, d.dtype);
        SNNHIP_REQUIRE(dims_match(in[0], d.N, d.H, d.W, d.C) && dims_match(out, d.N, d.H, d.W, d.C), "u16_in: tensor dims do not match the plan");
        const size_t pixels = static_cast<size_t>(d.N) * d.H * d.W;
        U16Affine f;
        for (int c = 0; c < 4; ++c) {
            f.a[c] = d.means[c];
            f.b[c] = d.norms[c];
        }
        f.maxval = 65535.0f;
        f.shift = d.shift;
        const unsigned g = grid_for(ctx, pixels / 4 + 1);
        const unsigned short* src = reinterpret_cast<const unsigned short*>(in[0]->data);
#define SNNHIP_U16_IN(CC) SNNHIP_LAUNCH((u16_in_kernel<CC, T>), dim3(g), dim3(256), 0, ctx->stream, pixels, f, src, mptr<T>(out))
        SNNHIP_WITH_T(out->dtype, if (d.C == 1) SNNHIP_U16_IN(1); else if (d.C == 2) SNNHIP_U16_IN(2); else if (d.C == 3) SNNHIP_U16_IN(3); else SNNHIP_U16_IN(4););
#undef SNNHIP_U16_IN
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }
};

struct U16OutPlan : snnhip_plan {
    snnhip_u16_out_desc d;
    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        SNNHIP_REQUIRE(nIn == 1, "u16_out: expects 1 input, got %d", nIn);
        SNNHIP_REQUIRE(in[0]->dtype == d.dtype, "u16_out: input dtype %d, the plan was built for %d", in[0]->dtype, d.dtype);
        SNNHIP_REQUIRE(out->dtype == SNNHIP_U16, "u16_out: the output tensor must be SNNHIP_U16, got dtype %d", out->dtype);
        SNNHIP_REQUIRE(dims_match(in[0], d.N, d.H, d.W, d.C) && dims_match(out, d.N, d.H, d.W, d.C), "u16_out: tensor dims do not match the plan");
        const size_t pixels = static_cast<size_t>(d.N) * d.H * d.W;
        U16Affine f;
        for (int c = 0; c < 4; ++c) {
            f.a[c] = d.scale[c];
            f.b[c] = d.offset[c];
        }
        f.maxval = static_cast<float>(d.maxval); // (<= 65535: exact)
        f.shift = d.shift;
        const unsigned g = grid_for(ctx, pixels / 4 + 1);
        unsigned short* dst = reinterpret_cast<unsigned short*>(out->data);
#define SNNHIP_U16_OUT(CC) SNNHIP_LAUNCH((u16_out_kernel<CC, T>), dim3(g), dim3(256), 0, ctx->stream, pixels, f, cptr<T>(in[0]), dst)
        SNNHIP_WITH_T(in[0]->dtype, if (d.C == 1) SNNHIP_U16_OUT(1); else if (d.C == 2) SNNHIP_U16_OUT(2); else if (d.C == 3) SNNHIP_U16_OUT(3); else SNNHIP_U16_OUT(4););
#undef SNNHIP_U16_OUT
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }
};

} // namespace

bool u16_in_plan_desc(const snnhip_plan* plan, snnhip_u16_in_desc* d) {
    auto* p = dynamic_cast<const U16InPlan*>(plan);
    if (p && d) *d = p->d;
    return p != nullptr;
}

bool u16_out_plan_desc(const snnhip_plan* plan, snnhip_u16_out_desc* d) {
    auto* p = dynamic_cast<const U16OutPlan*>(plan);
    if (p && d) *d = p->d;
    return p != nullptr;
}

} // namespace snnhip

using namespace snnhip;

extern "C" {

int snnhip_u16_in_plan_create(snnhip_ctx* ctx, const snnhip_u16_in_desc* desc, snnhip_plan** out) {
    SNNHIP_REQUIRE(ctx && desc && out, "u16_in_plan_create: null argument");
    SNNHIP_REQUIRE(desc->N > 0 && desc->H > 0 && desc->W > 0, "u16_in desc: bad dims %dx%dx%d", desc->N, desc->H, desc->W);
    SNNHIP_REQUIRE(desc->C >= 1 && desc->C <= 4, "u16_in desc: %d channels (1..4: R16, RG16, RGB16, RGBA16)", desc->C);
    SNNHIP_REQUIRE(desc->dtype == SNNHIP_F32 || desc->dtype == SNNHIP_F16, "u16_in desc: dtype %d (SNNHIP_F32 or SNNHIP_F16)", desc->dtype);
    SNNHIP_REQUIRE(desc->shift >= 0 && desc->shift <= 15, "u16_in desc: shift %d (0..15)", desc->shift);
    auto* plan = new U16InPlan();
    plan->ctx = ctx;
    plan->dtype = desc->dtype;
    plan->rawInput = SNNHIP_U16;
    plan->d = *desc;
    for (int i = 0; i < 4; ++i) {
        plan->inDims[i] = plan->outDims[i] = (&desc->N)[i];
    }
    const double elems = static_cast<double>(desc->N) * desc->H * desc->W * desc->C;
    plan->bytes = elems * (2 + (desc->dtype == SNNHIP_F16 ? 2 : 4));
    char buf[128];
    snprintf(buf, sizeof(buf), "u16_in_%s c=%d %dx%d shift=%d kernel=u16_in_kernel", dtype_name(desc->dtype), desc->C, desc->H, desc->W, desc->shift);
    plan->desc = buf;
    *out = plan;
    return SNNHIP_OK;
}

int snnhip_u16_out_plan_create(snnhip_ctx* ctx, const snnhip_u16_out_desc* desc, snnhip_plan** out) {
    SNNHIP_REQUIRE(ctx && desc && out, "u16_out_plan_create: null argument");
    SNNHIP_REQUIRE(desc->N > 0 && desc->H > 0 && desc->W > 0, "u16_out desc: bad dims %dx%dx%d", desc->N, desc->H, desc->W);
    SNNHIP_REQUIRE(desc->C >= 1 && desc->C <= 4, "u16_out desc: %d channels (1..4: R16, RG16, RGB16, RGBA16)", desc->C);
    SNNHIP_REQUIRE(desc->dtype == SNNHIP_F32 || desc->dtype == SNNHIP_F16, "u16_out desc: dtype %d (SNNHIP_F32 or SNNHIP_F16)", desc->dtype);
    SNNHIP_REQUIRE(desc->maxval >= 1 && desc->maxval <= 65535, "u16_out desc: maxval %d (1..65535)", desc->maxval);
    SNNHIP_REQUIRE(desc->shift >= 0 && desc->shift <= 15, "u16_out desc: shift %d (0..15)", desc->shift);
    SNNHIP_REQUIRE((static_cast<long long>(desc->maxval) << desc->shift) <= 65535, "u16_out desc: maxval %d << shift %d does not fit 16 bits", desc->maxval, desc->shift);
    auto* plan = new U16OutPlan();
    plan->ctx = ctx;
    plan->dtype = desc->dtype;
    plan->rawOutput = SNNHIP_U16;
    plan->d = *desc;
    for (int i = 0; i < 4; ++i) {
        plan->inDims[i] = plan->outDims[i] = (&desc->N)[i];
    }
    const double elems = static_cast<double>(desc->N) * desc->H * desc->W * desc->C;
    plan->bytes = elems * (2 + (desc->dtype == SNNHIP_F16 ? 2 : 4));
    char buf[160];
    snprintf(buf, sizeof(buf), "u16_out_%s c=%d %dx%d maxval=%d shift=%d kernel=u16_out_kernel", dtype_name(desc->dtype), desc->C, desc->H, desc->W, desc->maxval, desc->shift);
    plan->desc = buf;
    *out = plan;
    return SNNHIP_OK;
}

} // extern "C"
