// frame_tensor_yuv.hip -- the output tensor of an RGB(A) model straight to the planes of a 4:2:0 video frame of the same extent (include/snnhip.h:
// snnhip_tensor_yuv_plan_create / snnhip_tensor_yuv_planar_plan_create / snnhip_tensor_yuv_coefficients / snnhip_plan_run_io):
// what an encoder takes behind a style or enhancement network.  The inverse of frame_yuv_tensor.hip.  The reference has nothing for this: the libyuv it
// vendors converts on the CPU.
//
//   tensor_yuv:  T [N][H][W][C] (T = float or half, C = 3 or 4, channel 3 ignored) -> the luma plane E [N][H][W][1] and the chroma E [N][H/2][W/2][2],
//                interleaved CbCr.  p_c = clamp(fmaf(x_c, scale[c], offset[c]), 0, maxval); ylo = luma_f32(p); Y = Yoff + ys ylo; dB = B - ylo,
//                dR = R - ylo decimated 2 x 2 (rows 1/2, 1/2; columns 1/2, 1/2 for centred chroma, 1/4, 1/2, 1/4 over 2I - 1 .. 2I + 1 for left-sited
//                chroma, column -1 clamped to 0), horizontal first; Cb = Coff + cbs dB~, Cr = Coff + crs dR~; q = clamp(rint(.), 0, maxval) << shift.
//   tensor_yuv_planar:  the same with the chroma as two planes E [2N][H/2][W/2][1] (I420 / I010); only the chroma store differs.
//
// One launch, output-centric, no LDS, no barrier, no intermediate frame.  The strips of a frame -- two luma rows by S columns, S = tensor_yuv_strip --
// are one flat run of N * H/2 * ceil(W / S) and a lane owns one of them: it loads the two rows of S pixels as dwords, two pixels at a time (a pair of
// pixels is 3, 4, 6 or 8 dwords and starts on a dword for every even column), converts them, stores each luma row and each chroma row as whole dwords
// and needs nothing from its neighbours: the left-sited filter's column 2I - 1 at the strip's left edge is one more pixel, loaded by elements by the
// same lane.  A run that is short (the last strip of a row whose W is no multiple of S) or does not start on a dword (W not a multiple of 4 puts every
// other 8-bit row 2 bytes off) is stored by elements under a guard; pixel pairs past the row's end are not loaded.  The decimation weights are powers of
// two, so the filter needs no table; contraction is off in the arithmetic and every fused multiply-add is written out, and the shared luma function is
// evaluated one pixel at a time (ty_pixel), so that the sixteen instances give the same bits.
#include "frame_tensor_yuv.h"
#include "plan_util.h"
#include "snnhip_internal.h"

namespace snnhip {
namespace {

struct TensorYuvParams {
    int N, H, W;     // the tensor's extent = the luma plane's
    int CH, CW;      // the chroma plane(s): H / 2, W / 2
    unsigned SW;     // strips per pair of rows: ceil(W / S)
    unsigned strips; // N * CH * SW
    int shift, left;
    float maxval;
    float kr, kg, kb;
    TensorYuvCoeffs m;
    float scale[3], offset[3];
};

// NW dwords (any number) from a dword-aligned address, four at a time
template <int NW>
__device__ __forceinline__ void load_run(const void* p, unsigned* w) {
    if constexpr (NW > 4) {
        load_words<4>(p, w);
        load_run<NW - 4>(reinterpret_cast<const unsigned*>(p) + 4, w + 4);
    } else {
        load_words<NW>(p, w);
    }
}

// element e of a run of T held as dwords, widened to float
template <typename T>
__device__ __forceinline__ float tensor_elem(const unsigned* w, int e) {
    if constexpr (sizeof(T) == 4) return __uint_as_float(w[e]);
    else return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<unsigned short>((w[e / 2] >> (16 * (e % 2))) & 0xffffu)));
}

// one pixel x (R, G, B as the tensor holds them): the luma code, and the two unquantised chroma differences
__device__ __forceinline__ void ty_pixel(const TensorYuvParams& P, const float (&x)[3], unsigned* yq, float* dB, float* dR) {
#pragma clang fp contract(off)
    float p[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = fminf(fmaxf(__builtin_fmaf(x[c], P.scale[c], P.offset[c]), 0.0f), P.maxval);
    // One pixel's luma at a time, between two empty statements that pin its operands and its result to registers of their own: luma_f32 is the shared
    // function and is contracted as the compiler sees fit, and without the pins an instance that holds more pixels per lane packs the products of two
    // pixels into one instruction and fuses them another way (seen: a luma code one apart between the planar and the interleaved plan on a near tie).
    // With them the sixteen instances, and a strip's own pixel and its neighbour's edge pixel, evaluate it with the same roundings.
    asm volatile("" : "+v"(p[0]), "+v"(p[1]), "+v"(p[2]));
    float ylo = luma_f32(p[0], p[1], p[2], P.kr, P.kg, P.kb);
    asm volatile("" : "+v"(ylo));
    if (yq) *yq = quantize_frame(__builtin_fmaf(P.m.ys, ylo, P.m.yoff), P.maxval) << P.shift;
    *dB = p[2] - ylo;
    *dR = p[0] - ylo;
}

// NE values to dst as E: whole dwords when all of them are there and dst is on a dword, else the `valid` first ones element by element
template <typename E, int NE>
__device__ __forceinline__ void store_run(E* dst, const unsigned (&q)[NE], int valid) {
    constexpr int PER = 4 / static_cast<int>(sizeof(E)), NW = NE / PER, BITS = 8 * static_cast<int>(sizeof(E));
    static_assert(NW * PER == NE, "a full run is whole dwords");
    if (valid == NE && (reinterpret_cast<size_t>(dst) & 3) == 0) {
        unsigned w[NW];
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            w[k] = 0;
#pragma unroll
            for (int j = 0; j < PER; ++j) w[k] |= q[k * PER + j] << (BITS * j);
        }
        store_words<NW>(dst, w);
    } else {
#pragma unroll
        for (int i = 0; i < NE; ++i)
            if (i < valid) dst[i] = static_cast<E>(q[i]);
    }
}

template <typename T, int C, typename E, bool PLANAR>
__device__ __forceinline__ void tensor_yuv_body(const TensorYuvParams& P, const T* __restrict__ src, E* __restrict__ luma, E* __restrict__ chroma) {
#pragma clang fp contract(off)
    constexpr int S = tensor_yuv_strip(static_cast<int>(sizeof(E)), PLANAR), HS = S / 2;
    constexpr int PW = 2 * C * static_cast<int>(sizeof(T)) / 4; // dwords of a pair of pixels
    const unsigned s = blockIdx.x * static_cast<unsigned>(kTensorYuvThreads) + threadIdx.x; // strips < 2^31 (checked by the plan)
    if (s >= P.strips) return;                                                             // (no barrier anywhere below)
    const int x0 = static_cast<int>(s % P.SW) * S;
    const unsigned r = s / P.SW;
    const int J = static_cast<int>(r % static_cast<unsigned>(P.CH));
    const size_t n = r / static_cast<unsigned>(P.CH);
    const int valid = min(S, P.W - x0); // even, at least 2
    float hb[2][HS], hr[2][HS];         // the two rows, filtered horizontally
#pragma unroll
    for (int row = 0; row < 2; ++row) {
        const size_t pix = (n * P.H + static_cast<size_t>(2 * J + row)) * P.W; // first pixel of the row
        const T* rowp = src + (pix + x0) * C;
        unsigned yq[S];
        float dB[S + 1], dR[S + 1]; // [0]: column x0 - 1 (left-sited chroma only)
#pragma unroll
        for (int pr = 0; pr < HS; ++pr) {
            unsigned w[PW];
#pragma unroll
            for (int k = 0; k < PW; ++k) w[k] = 0;
            if (2 * pr < valid) load_run<PW>(rowp + 2 * pr * C, w); // (a pair past the row's end stays zero: it is converted and filtered like the others, and nothing of it is stored)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float x[3] = {tensor_elem<T>(w, j * C), tensor_elem<T>(w, j * C + 1), tensor_elem<T>(w, j * C + 2)};
                ty_pixel(P, x, &yq[2 * pr + j], &dB[1 + 2 * pr + j], &dR[1 + 2 * pr + j]);
            }
        }
        store_run<E, S>(luma + pix + x0, yq, valid);
        if (P.left) {
            const T* e = src + (pix + static_cast<size_t>(max(x0 - 1, 0))) * C;
            const float x[3] = {static_cast<float>(e[0]), static_cast<float>(e[1]), static_cast<float>(e[2])};
            ty_pixel(P, x, nullptr, &dB[0], &dR[0]);
#pragma unroll
            for (int i = 0; i < HS; ++i) {
                hb[row][i] = (0.25f * dB[2 * i] + 0.5f * dB[2 * i + 1]) + 0.25f * dB[2 * i + 2];
                hr[row][i] = (0.25f * dR[2 * i] + 0.5f * dR[2 * i + 1]) + 0.25f * dR[2 * i + 2];
            }
        } else {
#pragma unroll
            for (int i = 0; i < HS; ++i) {
                hb[row][i] = 0.5f * dB[2 * i + 1] + 0.5f * dB[2 * i + 2];
                hr[row][i] = 0.5f * dR[2 * i + 1] + 0.5f * dR[2 * i + 2];
            }
        }
    }
    unsigned cb[HS], cr[HS];
#pragma unroll
    for (int i = 0; i < HS; ++i) {
        cb[i] = quantize_frame(__builtin_fmaf(P.m.cbs, 0.5f * hb[0][i] + 0.5f * hb[1][i], P.m.coff), P.maxval) << P.shift;
        cr[i] = quantize_frame(__builtin_fmaf(P.m.crs, 0.5f * hr[0][i] + 0.5f * hr[1][i], P.m.coff), P.maxval) << P.shift;
    }
    const size_t plane = static_cast<size_t>(P.CH) * P.CW;
    const size_t at = static_cast<size_t>(J) * P.CW + x0 / 2;
    if constexpr (PLANAR) {
        store_run<E, HS>(chroma + 2 * n * plane + at, cb, valid / 2);
        store_run<E, HS>(chroma + (2 * n + 1) * plane + at, cr, valid / 2);
    } else {
        unsigned q[S];
#pragma unroll
        for (int i = 0; i < HS; ++i) q[2 * i] = cb[i], q[2 * i + 1] = cr[i];
        store_run<E, S>(chroma + (n * plane + at) * 2, q, valid);
    }
}

template <typename T, int C, typename E>
__global__ __launch_bounds__(kTensorYuvThreads) void tensor_yuv_kernel(TensorYuvParams P, const T* __restrict__ src, E* __restrict__ luma, E* __restrict__ cbcr) {
    tensor_yuv_body<T, C, E, false>(P, src, luma, cbcr);
}

template <typename T, int C, typename E>
__global__ __launch_bounds__(kTensorYuvThreads) void tensor_yuv_planar_kernel(TensorYuvParams P, const T* __restrict__ src, E* __restrict__ luma, E* __restrict__ chroma) {
    tensor_yuv_body<T, C, E, true>(P, src, luma, chroma);
}

struct TensorYuvPlan : snnhip_plan {
    snnhip_tensor_yuv_desc d;
    TensorYuvParams P;
    bool planar = false; // the chroma output is [2N][H/2][W/2][1] (snnhip_tensor_yuv_planar_plan_create)
    const char* name() const { return planar ? "tensor_yuv_planar" : "tensor_yuv"; }

    template <typename T, int C, typename E>
    void launch_one(const snnhip_tensor* in, snnhip_tensor* y, snnhip_tensor* c) {
        const dim3 grid((P.strips + kTensorYuvThreads - 1) / kTensorYuvThreads);
        const T* src = reinterpret_cast<const T*>(in->data);
        E* ydst = reinterpret_cast<E*>(y->data);
        E* cdst = reinterpret_cast<E*>(c->data);
        if (planar) SNNHIP_LAUNCH((tensor_yuv_planar_kernel<T, C, E>), grid, dim3(kTensorYuvThreads), 0, ctx->stream, P, src, ydst, cdst);
        else SNNHIP_LAUNCH((tensor_yuv_kernel<T, C, E>), grid, dim3(kTensorYuvThreads), 0, ctx->stream, P, src, ydst, cdst);
    }
    template <typename T, typename E>
    void launch_c(const snnhip_tensor* in, snnhip_tensor* y, snnhip_tensor* c) {
        if (d.C == 3) launch_one<T, 3, E>(in, y, c);
        else launch_one<T, 4, E>(in, y, c);
    }
    template <typename E>
    void launch(const snnhip_tensor* in, snnhip_tensor* y, snnhip_tensor* c) {
        if (d.in_dtype == SNNHIP_F16) launch_c<_Float16, E>(in, y, c);
        else launch_c<float, E>(in, y, c);
    }

    int run(const snnhip_tensor* const*, int, snnhip_tensor*) override {
        set_error("%s: the plan has two outputs (the luma plane, the chroma): run it with snnhip_plan_run_io", name());
        return SNNHIP_E_INVALID;
    }

    int runIO(const snnhip_tensor* const* in, int nIn, snnhip_tensor* const* out, int nOut) override {
        const char* nm = name();
        SNNHIP_REQUIRE(nIn == 1, "%s: expects 1 input (the model's output tensor), got %d", nm, nIn);
        SNNHIP_REQUIRE(nOut == 2, "%s: expects 2 outputs (the luma plane, the chroma), got %d", nm, nOut);
        SNNHIP_REQUIRE(in[0]->dtype == d.in_dtype, "%s: the input must have dtype %d, got %d", nm, d.in_dtype, in[0]->dtype);
        SNNHIP_REQUIRE(out[0]->dtype == d.out_dtype && out[1]->dtype == d.out_dtype, "%s: both outputs must have dtype %d, got %d and %d", nm, d.out_dtype, out[0]->dtype,
                       out[1]->dtype);
        SNNHIP_REQUIRE(dims_match(in[0], d.N, d.H, d.W, d.C), "%s: the input is %dx%dx%dx%d, the plan was built for %dx%dx%dx%d", nm, in[0]->n, in[0]->h, in[0]->w, in[0]->c, d.N,
                       d.H, d.W, d.C);
        SNNHIP_REQUIRE(dims_match(out[0], d.N, d.H, d.W, 1), "%s: the luma plane is %dx%dx%dx%d, the plan was built for %dx%dx%dx1", nm, out[0]->n, out[0]->h, out[0]->w, out[0]->c,
                       d.N, d.H, d.W);
        if (planar)
            SNNHIP_REQUIRE(dims_match(out[1], 2 * d.N, d.H / 2, d.W / 2, 1),
                           "%s: the chroma tensor is %dx%dx%dx%d, the plan was built for %dx%dx%dx1 ([2N][H/2][W/2][1]: plane 2n is Cb, 2n + 1 Cr of image n)", nm, out[1]->n, out[1]->h,
                           out[1]->w, out[1]->c, 2 * d.N, d.H / 2, d.W / 2);
        else
            SNNHIP_REQUIRE(dims_match(out[1], d.N, d.H / 2, d.W / 2, 2), "%s: the chroma plane is %dx%dx%dx%d, the plan was built for %dx%dx%dx2", nm, out[1]->n, out[1]->h, out[1]->w,
                           out[1]->c, d.N, d.H / 2, d.W / 2);
        SNNHIP_REQUIRE(((reinterpret_cast<size_t>(in[0]->data) | reinterpret_cast<size_t>(out[0]->data) | reinterpret_cast<size_t>(out[1]->data)) & 3) == 0,
                       "%s: the input and both outputs must start on a dword", nm);
        if (d.out_dtype == SNNHIP_U8) launch<unsigned char>(in[0], out[0], out[1]);
        else launch<unsigned short>(in[0], out[0], out[1]);
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }
};

} // namespace
} // namespace snnhip

using namespace snnhip;

extern "C" {

int snnhip_tensor_yuv_coefficients(int maxval, int range, float kr, float kb, float* out, int capacity) {
    SNNHIP_REQUIRE(out, "tensor_yuv_coefficients: null argument");
    SNNHIP_REQUIRE(capacity >= 5, "tensor_yuv_coefficients: room for %d floats, 5 needed", capacity);
    SNNHIP_REQUIRE(maxval >= 255 && maxval <= 65535 && (maxval + 1) % 256 == 0, "tensor_yuv_coefficients: maxval %d (maxval + 1 must be a multiple of 256)", maxval);
    SNNHIP_REQUIRE(range == SNNHIP_RANGE_LIMITED || range == SNNHIP_RANGE_FULL, "tensor_yuv_coefficients: range %d (SNNHIP_RANGE_LIMITED or SNNHIP_RANGE_FULL)", range);
    SNNHIP_REQUIRE(matrix_ok(kr, kb), "tensor_yuv_coefficients: kr = %g, kb = %g (0 < kr, 0 < kb, kr + kb < 1)", kr, kb);
    const TensorYuvCoeffs c = tensor_yuv_coeffs(maxval, range, kr, kb);
    out[0] = c.yoff, out[1] = c.ys, out[2] = c.coff, out[3] = c.cbs, out[4] = c.crs;
    return SNNHIP_OK;
}

// snnhip_tensor_yuv_plan_create and snnhip_tensor_yuv_planar_plan_create: one desc, one set of checks and coefficients
static int tensor_yuv_plan_make(snnhip_ctx* ctx, const snnhip_tensor_yuv_desc* desc, snnhip_plan** out, bool planar) {
    SNNHIP_REQUIRE(ctx && desc && out, "%s: null argument", planar ? "tensor_yuv_planar_plan_create" : "tensor_yuv_plan_create");
    SNNHIP_REQUIRE(desc->N >= 1 && desc->H > 0 && desc->W > 0, "tensor_yuv desc: bad dims %dx%dx%d", desc->N, desc->H, desc->W);
    SNNHIP_REQUIRE(desc->H % 2 == 0 && desc->W % 2 == 0, "tensor_yuv desc: a %dx%d tensor: both extents of a 4:2:0 frame must be even", desc->H, desc->W);
    SNNHIP_REQUIRE(desc->C == 3 || desc->C == 4, "tensor_yuv desc: %d channels (3: RGB, 4: RGB and an ignored fourth)", desc->C);
    SNNHIP_REQUIRE(desc->in_dtype == SNNHIP_F32 || desc->in_dtype == SNNHIP_F16, "tensor_yuv desc: in_dtype %d (SNNHIP_F32 or SNNHIP_F16)", desc->in_dtype);
    int bits = 0;
    const int fmt = check_sample_format("tensor_yuv desc", "frames", desc->out_dtype, desc->siting, desc->shift, desc->maxval, &bits);
    if (fmt != SNNHIP_OK) return fmt;
    SNNHIP_REQUIRE(desc->range == SNNHIP_RANGE_LIMITED || desc->range == SNNHIP_RANGE_FULL, "tensor_yuv desc: range %d (SNNHIP_RANGE_LIMITED or SNNHIP_RANGE_FULL)", desc->range);
    SNNHIP_REQUIRE((desc->maxval + 1) % 256 == 0, "tensor_yuv desc: maxval %d: maxval + 1 must be a multiple of 256 (the offsets 16k, 128k of the matrix are integers)", desc->maxval);
    SNNHIP_REQUIRE(matrix_ok(desc->kr, desc->kb), "tensor_yuv desc: kr = %g, kb = %g (0 < kr, 0 < kb, kr + kb < 1)", desc->kr, desc->kb);
    const int es = bits / 8, S = tensor_yuv_strip(es, planar);
    const bool half = desc->in_dtype == SNNHIP_F16;
    const double pixels = static_cast<double>(desc->N) * desc->H * desc->W;
    const double SW = (desc->W + S - 1) / S;
    const double strips = static_cast<double>(desc->N) * (desc->H / 2) * SW;
    SNNHIP_REQUIRE(strips < 2147483648.0 && pixels * desc->C < 9.0e15 && 2.0 * desc->N < 2147483648.0 && desc->H <= (1 << 30) && desc->W <= (1 << 30),
                   "tensor_yuv desc: %dx%dx%d is too large", desc->N, desc->H, desc->W);
    auto* plan = new TensorYuvPlan();
    plan->ctx = ctx;
    plan->numInputs = 1;
    plan->numOutputs = 2;
    plan->dtype = desc->in_dtype;
    plan->anyDtype = true; // a float tensor in, raw planes out: runIO() checks every position itself
    plan->rawOutput = desc->out_dtype;
    plan->d = *desc;
    plan->planar = planar;
    plan->P = TensorYuvParams{};
    plan->P.N = desc->N;
    plan->P.H = desc->H;
    plan->P.W = desc->W;
    plan->P.CH = desc->H / 2;
    plan->P.CW = desc->W / 2;
    plan->P.SW = static_cast<unsigned>(SW);
    plan->P.strips = static_cast<unsigned>(strips);
    plan->P.shift = desc->shift;
    plan->P.left = desc->siting == SNNHIP_SITING_LEFT;
    plan->P.maxval = static_cast<float>(desc->maxval);
    plan->P.kr = desc->kr;
    plan->P.kb = desc->kb;
    plan->P.kg = static_cast<float>(1.0 - static_cast<double>(desc->kr) - static_cast<double>(desc->kb)); // (as rgb_luma, ycc_merge and rgb_cbcr form it)
    plan->P.m = tensor_yuv_coeffs(desc->maxval, desc->range, desc->kr, desc->kb);
    for (int c = 0; c < 3; ++c) plan->P.scale[c] = desc->scale[c], plan->P.offset[c] = desc->offset[c];
    plan->inDims[0] = plan->outDims[0] = desc->N;
    plan->inDims[1] = plan->outDims[1] = desc->H;
    plan->inDims[2] = plan->outDims[2] = desc->W;
    plan->inDims[3] = desc->C;
    plan->outDims[3] = 1; // the luma plane; the chroma follows from it
    plan->bytes = pixels * desc->C * (half ? 2 : 4) + pixels * 1.5 * es; // the input once, both outputs once
    // per pixel: three maps (2 each) and their clamps, the luma (5), its code (2), two differences; per chroma sample (a quarter of a pixel) and
    // component: the horizontal filter of two rows (3 or 5 each), the vertical one (3), the code (2)
    plan->flops = pixels * (6.0 + 5.0 + 2.0 + 2.0 + 0.25 * 2.0 * (2.0 * (plan->P.left ? 5.0 : 3.0) + 5.0));
    char buf[320];
    snprintf(buf, sizeof(buf), "%s_u%d c=%d %s siting=%s range=%s %dx%d tile=%d maxval=%d shift=%d kr=%g kb=%g kernel=%s", plan->name(), bits, desc->C, half ? "f16" : "f32",
             plan->P.left ? "left" : "centre", desc->range == SNNHIP_RANGE_LIMITED ? "limited" : "full", desc->H, desc->W, tensor_yuv_tile(es, planar), desc->maxval, desc->shift,
             desc->kr, desc->kb, planar ? "tensor_yuv_planar_kernel" : "tensor_yuv_kernel");
    plan->desc = buf;
    *out = plan;
    return SNNHIP_OK;
}

int snnhip_tensor_yuv_plan_create(snnhip_ctx* ctx, const snnhip_tensor_yuv_desc* desc, snnhip_plan** out) { return tensor_yuv_plan_make(ctx, desc, out, false); }

int snnhip_tensor_yuv_planar_plan_create(snnhip_ctx* ctx, const snnhip_tensor_yuv_desc* desc, snnhip_plan** out) { return tensor_yuv_plan_make(ctx, desc, out, true); }

} // extern "C"
