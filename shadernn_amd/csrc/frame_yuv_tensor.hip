// frame_yuv_tensor.hip -- a 4:2:0 video frame straight to the normalised input tensor of an RGB(A) model, at the model's input size (include/snnhip.h:
// snnhip_yuv_tensor_plan_create / snnhip_yuv_tensor_planar_plan_create / snnhip_yuv_tensor_taps).  The reference converts and
// resizes decoded video on the CPU (the libyuv it vendors) and uploads floats.
//
//   yuv_tensor:  Y E [N][H][W][1] + CbCr E [N][H/2][W/2][2] -> T [N][OH][OW][C], T = float or half, C = 3 (R, G, B) or 4 (+ alpha).  The source pixel
//                at luma (Y, X) is yuv_rgb's value at r = 1 in front of its rounding, clamped to [0, maxval] as a float; output pixel (oy, ox) samples
//                it at resize's position, nearest or bilinear over the four clamped source pixels, from two host tables (no position arithmetic on
//                the device); t = (sample - mean) * norm.
//   yuv_tensor_planar:  the same with the chroma as two planes E [2N][H/2][W/2][1] (I420 / I010); only the chroma load differs.
//
// One launch, output-centric, no LDS, no barrier, no intermediate frame.  The output is one flat run of N * OH * OW pixels and a lane owns one of them
// (two for fp16 RGB, frame_yuv_tensor.h), so that every store is whole dwords from a dword boundary whatever OW is; the one exception is the single
// last pixel of an fp16 RGB tensor with an odd pixel count (a dword and a half).  Two instances per layout: SINGLE (NP = 1: nearest, and linear tables
// whose weights are all 0 -- ratio 1) evaluates one source pixel from a 5 x 5 chroma window; BILINEAR (NP = 2) evaluates the 2 x 2 adjacent source pixels
// from the 6 x 6 chroma window under them: every chroma row is filtered horizontally once for both source columns, then vertically for both source
// rows.  The window is addressed from the first source pixel; the second one's five weights sit at offset 0 or 1 of six (the sixth is 0), so that
// every register index is a compile-time constant and a term 0 * v adds exactly nothing: each source pixel sees yuv_rgb's five-term sums in
// yuv_rgb's order.  Contraction is off in the arithmetic and every fused multiply-add is written out (a product, then a chain of fmaf), so that the
// sixteen instances of a layout and the two layouts give the same bits.  A second source pixel on the same clamped index as the first is a copy of
// it, never a second evaluation.  Interleaved chroma is loaded one CbCr pixel per access (2 or 4 bytes, always aligned); everything else is element
// loads with clamped indices, which is what lets any even extent through without an edge path.  Measured: 1080p to
// 224 x 224 x 4, batch 32, in 35 us against 607 us for the three launches it replaces; 720p to 720p fp16 in 12 us against 23 us.
#include "frame_yuv_tensor.h"
#include "plan_util.h"
#include "snnhip_internal.h"

namespace snnhip {
namespace {

struct YuvTensorParams {
    int N, H, W;   // the luma plane
    int CH, CW;    // the chroma plane(s): H / 2, W / 2
    int OH, OW;
    unsigned pixels; // N * OH * OW
    int shift;
    float maxval;
    YuvRgbCoeffs m;
    float wh[2][5]; // yuv_rgb's tables at r = 1: [phase][offset -2 .. 2] along a row (the desc's siting) ...
    float wv[2][5]; // ... and along a column (centred)
    float mean[3], norm[3], alpha;
    const YuvTensorCoord* ty; // [OH]
    const YuvTensorCoord* tx; // [OW]
};

// chroma pixel `idx` (row * CW + column) of one image as (Cb, Cr) - Coff.  Interleaved: one access of the pair; planar: one element of each plane
template <typename E, bool PLANAR>
__device__ __forceinline__ void yt_chroma(const YuvTensorParams& P, const E* __restrict__ c0, const E* __restrict__ c1, size_t idx, float& cb, float& cr) {
    unsigned b, r;
    if constexpr (PLANAR) {
        b = c0[idx];
        r = c1[idx];
    } else if constexpr (sizeof(E) == 1) {
        const unsigned t = reinterpret_cast<const unsigned short*>(c0)[idx];
        b = t & 0xffu;
        r = t >> 8;
    } else {
        const unsigned t = reinterpret_cast<const unsigned*>(c0)[idx];
        b = t & 0xffffu;
        r = t >> 16;
    }
    cb = static_cast<float>(b >> P.shift) - P.m.coff;
    cr = static_cast<float>(r >> P.shift) - P.m.coff;
}

// v[qy][qx][c] = the source pixel at luma (Y[qy], X[qx]), channel c: yuv_rgb's expression at r = 1, not rounded, clamped to [0, maxval].
// X[1] >= X[0], Y[1] >= Y[0], at most one apart (the clamped i0, i1 of a table).
template <typename E, bool PLANAR, int NP>
__device__ __forceinline__ void yt_source(const YuvTensorParams& P, const E* __restrict__ yimg, const E* __restrict__ c0, const E* __restrict__ c1, const int (&Y)[NP],
                                          const int (&X)[NP], float (&v)[NP][NP][3]) {
#pragma clang fp contract(off) // every fused multiply-add below is written out: all instances (layouts, channels, output types) give the same bits
    constexpr int NT = 4 + NP; // the window: five chroma samples under one source pixel, six under two adjacent ones
    const int x0 = X[0] >> 1, y0 = Y[0] >> 1;
    float wx[NP][NT], wy[NP][NT];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const bool px = X[q] & 1, py = Y[q] & 1;
        const bool dx = (X[q] >> 1) != x0, dy = (Y[q] >> 1) != y0; // the second pixel lies over the next chroma sample
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const float hx0 = k < 5 ? (px ? P.wh[1][k < 5 ? k : 0] : P.wh[0][k < 5 ? k : 0]) : 0.0f;
            const float hx1 = k >= 1 ? (px ? P.wh[1][k - (k >= 1)] : P.wh[0][k - (k >= 1)]) : 0.0f;
            const float vy0 = k < 5 ? (py ? P.wv[1][k < 5 ? k : 0] : P.wv[0][k < 5 ? k : 0]) : 0.0f;
            const float vy1 = k >= 1 ? (py ? P.wv[1][k - (k >= 1)] : P.wv[0][k - (k >= 1)]) : 0.0f;
            wx[q][k] = dx ? hx1 : hx0;
            wy[q][k] = dy ? vy1 : vy0;
        }
    }
    int col[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) col[j] = min(max(x0 - 2 + j, 0), P.CW - 1);
    float hb[NT][NP], hr[NT][NP]; // the window's rows, filtered horizontally for each source column
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const size_t ro = static_cast<size_t>(min(max(y0 - 2 + i, 0), P.CH - 1)) * P.CW;
        float cb[NT], cr[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) yt_chroma<E, PLANAR>(P, c0, c1, ro + col[j], cb[j], cr[j]);
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            float ab = wx[q][0] * cb[0], ar = wx[q][0] * cr[0];
#pragma unroll
            for (int k = 1; k < NT; ++k) {
                ab = __builtin_fmaf(wx[q][k], cb[k], ab);
                ar = __builtin_fmaf(wx[q][k], cr[k], ar);
            }
            hb[i][q] = ab;
            hr[i][q] = ar;
        }
    }
#pragma unroll
    for (int qy = 0; qy < NP; ++qy) {
#pragma unroll
        for (int qx = 0; qx < NP; ++qx) {
            float cb = wy[qy][0] * hb[0][qx], cr = wy[qy][0] * hr[0][qx];
#pragma unroll
            for (int k = 1; k < NT; ++k) {
                cb = __builtin_fmaf(wy[qy][k], hb[k][qx], cb);
                cr = __builtin_fmaf(wy[qy][k], hr[k][qx], cr);
            }
            const unsigned u = yimg[static_cast<size_t>(Y[qy]) * P.W + X[qx]];
            const float yl = P.m.cy * (static_cast<float>(u >> P.shift) - P.m.yoff);
            const float e[3] = {__builtin_fmaf(P.m.crv, cr, yl), yl - __builtin_fmaf(P.m.cgv, cr, P.m.cgu * cb), __builtin_fmaf(P.m.cbu, cb, yl)};
#pragma unroll
            for (int c = 0; c < 3; ++c) v[qy][qx][c] = fminf(fmaxf(e[c], 0.0f), P.maxval);
        }
    }
    if constexpr (NP == 2) { // the same clamped index twice is one source pixel
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (X[1] == X[0]) v[0][1][c] = v[0][0][c], v[1][1][c] = v[1][0][c];
            if (Y[1] == Y[0]) v[1][0][c] = v[0][0][c], v[1][1][c] = v[0][1][c];
        }
    }
}

// flat output pixel p: t[0..2] = (sample - mean) * norm, t[3] = alpha
template <typename E, bool PLANAR, int NP>
__device__ __forceinline__ void yt_pixel(const YuvTensorParams& P, const E* __restrict__ luma, const E* __restrict__ chroma, unsigned p, float (&t)[4]) {
#pragma clang fp contract(off)
    const unsigned OW = static_cast<unsigned>(P.OW), OH = static_cast<unsigned>(P.OH);
    const unsigned ox = p % OW, r = p / OW;
    const unsigned oy = r % OH;
    const size_t n = r / OH;
    const YuvTensorCoord cy = P.ty[oy], cx = P.tx[ox];
    const size_t plane = static_cast<size_t>(P.CH) * P.CW;
    const E* yimg = luma + n * P.H * P.W;
    const E* c0 = PLANAR ? chroma + 2 * n * plane : chroma + n * plane * 2;
    const E* c1 = c0 + plane; // (read for planar chroma only)
    float s[3];
    if constexpr (NP == 1) {
        const int Y[1] = {cy.i0}, X[1] = {cx.i0};
        float v[1][1][3];
        yt_source<E, PLANAR, 1>(P, yimg, c0, c1, Y, X, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = v[0][0][c];
    } else {
        const int Y[2] = {cy.i0, cy.i1}, X[2] = {cx.i0, cx.i1};
        float v[2][2][3];
        yt_source<E, PLANAR, 2>(P, yimg, c0, c1, Y, X, v);
        const float ax = cx.a, ay = cy.a;
#pragma unroll
        for (int c = 0; c < 3; ++c) { // resize_kernel's form, horizontal first
            const float top = __builtin_fmaf(v[0][1][c], ax, v[0][0][c] * (1.0f - ax));
            const float bot = __builtin_fmaf(v[1][1][c], ax, v[1][0][c] * (1.0f - ax));
            s[c] = __builtin_fmaf(bot, ay, top * (1.0f - ay));
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = (s[c] - P.mean[c]) * P.norm[c];
    t[3] = P.alpha;
}

__device__ __forceinline__ unsigned half_bits(float f) { return __builtin_bit_cast(unsigned short, static_cast<_Float16>(f)); } // to nearest even

template <typename E, bool PLANAR, int NP, int C, bool HALF>
__device__ __forceinline__ void yuv_tensor_body(const YuvTensorParams& P, const E* __restrict__ luma, const E* __restrict__ chroma, void* __restrict__ out) {
    constexpr int LP = yuv_tensor_lane_pixels(C, HALF);
    const unsigned p0 = (blockIdx.x * static_cast<unsigned>(kYuvTensorThreads) + threadIdx.x) * LP; // pixels < 2^31 (checked by the plan)
    if (p0 >= P.pixels) return; // (no barrier anywhere below)
    float t[LP][4];
#pragma unroll
    for (int j = 0; j < LP; ++j) {
#pragma unroll
        for (int c = 0; c < 4; ++c) t[j][c] = 0.0f;
        if (p0 + j < P.pixels) yt_pixel<E, PLANAR, NP>(P, luma, chroma, p0 + j, t[j]);
    }
    if constexpr (!HALF) {
        unsigned w[C];
#pragma unroll
        for (int c = 0; c < C; ++c) w[c] = __float_as_uint(t[0][c]);
        store_words<C>(static_cast<float*>(out) + static_cast<size_t>(p0) * C, w);
    } else if constexpr (C == 4) {
        const unsigned w[2] = {half_bits(t[0][0]) | (half_bits(t[0][1]) << 16), half_bits(t[0][2]) | (half_bits(t[0][3]) << 16)};
        store_words<2>(static_cast<unsigned short*>(out) + static_cast<size_t>(p0) * 4, w);
    } else { // fp16 RGB: p0 is even, the pair starts 12 * (p0 / 2) bytes into the tensor
        unsigned short* dst = static_cast<unsigned short*>(out) + static_cast<size_t>(p0) * 3;
        const unsigned w[3] = {half_bits(t[0][0]) | (half_bits(t[0][1]) << 16), half_bits(t[0][2]) | (half_bits(t[1][0]) << 16), half_bits(t[1][1]) | (half_bits(t[1][2]) << 16)};
        if (p0 + 1 < P.pixels) {
            store_words<3>(dst, w);
        } else { // the last pixel of a tensor with an odd number of them: 6 bytes
            store_words<1>(dst, w);
            dst[2] = static_cast<unsigned short>(w[1] & 0xffffu);
        }
    }
}

template <typename E, int NP, int C, bool HALF>
__global__ __launch_bounds__(kYuvTensorThreads) void yuv_tensor_kernel(YuvTensorParams P, const E* __restrict__ luma, const E* __restrict__ cbcr, void* __restrict__ out) {
    yuv_tensor_body<E, false, NP, C, HALF>(P, luma, cbcr, out);
}

template <typename E, int NP, int C, bool HALF>
__global__ __launch_bounds__(kYuvTensorThreads) void yuv_tensor_planar_kernel(YuvTensorParams P, const E* __restrict__ luma, const E* __restrict__ chroma, void* __restrict__ out) {
    yuv_tensor_body<E, true, NP, C, HALF>(P, luma, chroma, out);
}

struct YuvTensorPlan : snnhip_plan {
    snnhip_yuv_tensor_desc d;
    YuvTensorParams P;
    bool planar = false; // the chroma input is [2N][H/2][W/2][1] (snnhip_yuv_tensor_planar_plan_create)
    bool single = false; // one source pixel per output pixel: nearest, or linear tables whose weights are all 0
    const char* name() const { return planar ? "yuv_tensor_planar" : "yuv_tensor"; }

    template <typename E, int NP, int C, bool HALF>
    void launch_one(const snnhip_tensor* y, const snnhip_tensor* c, snnhip_tensor* out) {
        const unsigned tile = static_cast<unsigned>(yuv_tensor_tile(C, HALF));
        const dim3 grid((P.pixels + tile - 1) / tile);
        const E* ysrc = reinterpret_cast<const E*>(y->data);
        const E* csrc = reinterpret_cast<const E*>(c->data);
        void* dst = out->data;
        if (planar) SNNHIP_LAUNCH((yuv_tensor_planar_kernel<E, NP, C, HALF>), grid, dim3(kYuvTensorThreads), 0, ctx->stream, P, ysrc, csrc, dst);
        else SNNHIP_LAUNCH((yuv_tensor_kernel<E, NP, C, HALF>), grid, dim3(kYuvTensorThreads), 0, ctx->stream, P, ysrc, csrc, dst);
    }
    template <typename E, int NP>
    void launch_np(const snnhip_tensor* y, const snnhip_tensor* c, snnhip_tensor* out) {
        const bool half = d.out_dtype == SNNHIP_F16;
        if (d.C == 3) {
            if (half) launch_one<E, NP, 3, true>(y, c, out);
            else launch_one<E, NP, 3, false>(y, c, out);
        } else {
            if (half) launch_one<E, NP, 4, true>(y, c, out);
            else launch_one<E, NP, 4, false>(y, c, out);
        }
    }
    template <typename E>
    void launch(const snnhip_tensor* y, const snnhip_tensor* c, snnhip_tensor* out) {
        if (single) launch_np<E, 1>(y, c, out);
        else launch_np<E, 2>(y, c, out);
    }

    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        const char* nm = name();
        SNNHIP_REQUIRE(nIn == 2, "%s: expects 2 inputs (the luma plane, the chroma tensor), got %d", nm, nIn);
        SNNHIP_REQUIRE(in[0]->dtype == d.src_dtype && in[1]->dtype == d.src_dtype, "%s: both inputs must have dtype %d, got %d and %d", nm, d.src_dtype, in[0]->dtype,
                       in[1]->dtype);
        SNNHIP_REQUIRE(out->dtype == d.out_dtype, "%s: the output must have dtype %d, got %d", nm, d.out_dtype, out->dtype);
        SNNHIP_REQUIRE(dims_match(in[0], d.N, d.H, d.W, 1), "%s: the luma plane is %dx%dx%dx%d, the plan was built for %dx%dx%dx1", nm, in[0]->n, in[0]->h, in[0]->w, in[0]->c, d.N,
                       d.H, d.W);
        if (planar)
            SNNHIP_REQUIRE(dims_match(in[1], 2 * d.N, d.H / 2, d.W / 2, 1),
                           "%s: the chroma tensor is %dx%dx%dx%d, the plan was built for %dx%dx%dx1 ([2N][H/2][W/2][1]: plane 2n is Cb, 2n + 1 Cr of image n)", nm, in[1]->n, in[1]->h,
                           in[1]->w, in[1]->c, 2 * d.N, d.H / 2, d.W / 2);
        else
            SNNHIP_REQUIRE(dims_match(in[1], d.N, d.H / 2, d.W / 2, 2), "%s: the chroma plane is %dx%dx%dx%d, the plan was built for %dx%dx%dx2", nm, in[1]->n, in[1]->h, in[1]->w,
                           in[1]->c, d.N, d.H / 2, d.W / 2);
        SNNHIP_REQUIRE(dims_match(out, d.N, d.OH, d.OW, d.C), "%s: the output is %dx%dx%dx%d, the plan was built for %dx%dx%dx%d", nm, out->n, out->h, out->w, out->c, d.N, d.OH,
                       d.OW, d.C);
        SNNHIP_REQUIRE(((reinterpret_cast<size_t>(in[1]->data) | reinterpret_cast<size_t>(out->data)) & 3) == 0, "%s: the chroma tensor and the output must start on a dword", nm);
        if (d.src_dtype == SNNHIP_U8) launch<unsigned char>(in[0], in[1], out);
        else launch<unsigned short>(in[0], in[1], out);
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }
};

int upload_coords(snnhip_plan* plan, int in, int out, int filter, const YuvTensorCoord** dev, bool* allZero) {
    std::vector<float> a(static_cast<size_t>(out));
    std::vector<int> idx(2 * static_cast<size_t>(out));
    const int rc = snnhip_yuv_tensor_taps(in, out, filter, a.data(), idx.data(), out);
    if (rc != SNNHIP_OK) return rc;
    std::vector<YuvTensorCoord> t(static_cast<size_t>(out));
    for (int o = 0; o < out; ++o) {
        SNNHIP_REQUIRE(idx[2 * o] >= 0 && idx[2 * o] <= idx[2 * o + 1] && idx[2 * o + 1] <= idx[2 * o] + 1 && idx[2 * o + 1] < in, "yuv_tensor: coordinate %d reads %d, %d of %d", o,
                       idx[2 * o], idx[2 * o + 1], in);
        t[o] = YuvTensorCoord{idx[2 * o], idx[2 * o + 1], a[o], 0};
        if (a[o] != 0.0f) *allZero = false;
    }
    static_assert(sizeof(YuvTensorCoord) == 4 * sizeof(float), "a coordinate is four dwords");
    float* p = nullptr;
    const int up = plan->upload(reinterpret_cast<const float*>(t.data()), t.size() * 4, &p); // (a byte copy)
    if (up != SNNHIP_OK) return up;
    *dev = reinterpret_cast<const YuvTensorCoord*>(p);
    return SNNHIP_OK;
}

} // namespace
} // namespace snnhip

using namespace snnhip;

extern "C" {

int snnhip_yuv_tensor_taps(int in, int out, int filter, float* weight, int* index, int capacity) {
#pragma clang fp contract(off)
    SNNHIP_REQUIRE(weight && index, "yuv_tensor_taps: null argument");
    SNNHIP_REQUIRE(in >= 1 && out >= 1 && in <= (1 << 30) && out <= (1 << 30), "yuv_tensor_taps: %d inputs, %d outputs (1 .. 2^30 each)", in, out);
    SNNHIP_REQUIRE(filter == SNNHIP_YUV_TENSOR_NEAREST || filter == SNNHIP_YUV_TENSOR_LINEAR, "yuv_tensor_taps: filter %d (SNNHIP_YUV_TENSOR_NEAREST or SNNHIP_YUV_TENSOR_LINEAR)",
                   filter);
    SNNHIP_REQUIRE(capacity >= out, "yuv_tensor_taps: room for %d coordinates, %d needed", capacity, out);
    const long long den = 2ll * out;
    for (int o = 0; o < out; ++o) {
        if (filter == SNNHIP_YUV_TENSOR_NEAREST) {
            const int i = static_cast<int>(((2ll * o + 1) * in) / den); // 0 .. in - 1
            index[2 * o] = index[2 * o + 1] = i;
            weight[o] = 0.0f;
        } else { // u = (o + 1/2) in / out - 1/2 = num / den, exactly
            const long long num = (2ll * o + 1) * in - out;
            long long i0 = num / den;
            if (num < 0 && i0 * den != num) --i0; // floor
            weight[o] = static_cast<float>(static_cast<double>(num - i0 * den) / static_cast<double>(den));
            index[2 * o] = static_cast<int>(i0 < 0 ? 0 : i0 > in - 1 ? in - 1 : i0);
            index[2 * o + 1] = static_cast<int>(i0 + 1 < 0 ? 0 : i0 + 1 > in - 1 ? in - 1 : i0 + 1);
        }
    }
    return SNNHIP_OK;
}

// snnhip_yuv_tensor_plan_create and snnhip_yuv_tensor_planar_plan_create: one desc, one set of checks, tables and coefficients
static int yuv_tensor_plan_make(snnhip_ctx* ctx, const snnhip_yuv_tensor_desc* desc, snnhip_plan** out, bool planar) {
    SNNHIP_REQUIRE(ctx && desc && out, "%s: null argument", planar ? "yuv_tensor_planar_plan_create" : "yuv_tensor_plan_create");
    SNNHIP_REQUIRE(desc->N > 0 && desc->H > 0 && desc->W > 0, "yuv_tensor desc: bad dims %dx%dx%d", desc->N, desc->H, desc->W);
    SNNHIP_REQUIRE(desc->H % 2 == 0 && desc->W % 2 == 0, "yuv_tensor desc: a %dx%d luma plane: both extents of a 4:2:0 frame must be even", desc->H, desc->W);
    SNNHIP_REQUIRE(desc->OH >= 1 && desc->OW >= 1, "yuv_tensor desc: a %dx%d output (at least 1x1)", desc->OH, desc->OW);
    SNNHIP_REQUIRE(desc->C == 3 || desc->C == 4, "yuv_tensor desc: %d channels (3: RGB, 4: RGB + alpha)", desc->C);
    SNNHIP_REQUIRE(desc->filter == SNNHIP_YUV_TENSOR_NEAREST || desc->filter == SNNHIP_YUV_TENSOR_LINEAR, "yuv_tensor desc: filter %d (SNNHIP_YUV_TENSOR_NEAREST or SNNHIP_YUV_TENSOR_LINEAR)",
                   desc->filter);
    SNNHIP_REQUIRE(desc->out_dtype == SNNHIP_F32 || desc->out_dtype == SNNHIP_F16, "yuv_tensor desc: out_dtype %d (SNNHIP_F32 or SNNHIP_F16)", desc->out_dtype);
    int bits = 0;
    const int fmt = check_sample_format("yuv_tensor desc", "frames", desc->src_dtype, desc->siting, desc->shift, desc->maxval, &bits);
    if (fmt != SNNHIP_OK) return fmt;
    SNNHIP_REQUIRE(desc->range == SNNHIP_RANGE_LIMITED || desc->range == SNNHIP_RANGE_FULL, "yuv_tensor desc: range %d (SNNHIP_RANGE_LIMITED or SNNHIP_RANGE_FULL)", desc->range);
    SNNHIP_REQUIRE((desc->maxval + 1) % 256 == 0, "yuv_tensor desc: maxval %d: maxval + 1 must be a multiple of 256 (the offsets 16k, 128k of the matrix are integers)", desc->maxval);
    SNNHIP_REQUIRE(matrix_ok(desc->kr, desc->kb), "yuv_tensor desc: kr = %g, kb = %g (0 < kr, 0 < kb, kr + kb < 1)", desc->kr, desc->kb);
    const bool half = desc->out_dtype == SNNHIP_F16;
    const double srcElems = static_cast<double>(desc->N) * desc->H * desc->W * 1.5; // the luma plane and half as many chroma samples
    const double outPixels = static_cast<double>(desc->N) * desc->OH * desc->OW;
    SNNHIP_REQUIRE(outPixels < 2147483648.0 && srcElems < 9.0e15 && 2.0 * desc->N < 2147483648.0 && desc->OH <= (1 << 30) && desc->OW <= (1 << 30) && desc->H <= (1 << 30) &&
                       desc->W <= (1 << 30),
                   "yuv_tensor desc: %dx%dx%d -> %dx%d is too large", desc->N, desc->H, desc->W, desc->OH, desc->OW);
    float wh[8] = {0}, wv[8] = {0};
    int bh[2] = {0}, bv[2] = {0};
    int rc = snnhip_bicubic_taps_420(1, desc->siting, wh, bh, 8);
    if (rc == SNNHIP_OK) rc = snnhip_bicubic_taps_420(1, SNNHIP_SITING_CENTRE, wv, bv, 8);
    if (rc != SNNHIP_OK) return rc;
    auto* plan = new YuvTensorPlan();
    plan->ctx = ctx;
    plan->numInputs = 2;
    plan->dtype = desc->out_dtype;
    plan->anyDtype = true; // raw frames in, a float tensor out: run() checks every position itself
    plan->rawInput = desc->src_dtype;
    plan->d = *desc;
    plan->planar = planar;
    plan->P = YuvTensorParams{};
    bool allZero = true;
    rc = upload_coords(plan, desc->H, desc->OH, desc->filter, &plan->P.ty, &allZero);
    if (rc == SNNHIP_OK) rc = upload_coords(plan, desc->W, desc->OW, desc->filter, &plan->P.tx, &allZero);
    if (rc != SNNHIP_OK) {
        delete plan;
        return rc;
    }
    plan->single = allZero;
    plan->P.N = desc->N;
    plan->P.H = desc->H;
    plan->P.W = desc->W;
    plan->P.CH = desc->H / 2;
    plan->P.CW = desc->W / 2;
    plan->P.OH = desc->OH;
    plan->P.OW = desc->OW;
    plan->P.pixels = static_cast<unsigned>(outPixels);
    plan->P.shift = desc->shift;
    plan->P.maxval = static_cast<float>(desc->maxval);
    plan->P.m = yuv_rgb_coeffs(desc->maxval, desc->range, desc->kr, desc->kb);
    widen_taps(2, wh, bh, plan->P.wh);
    widen_taps(2, wv, bv, plan->P.wv);
    for (int c = 0; c < 3; ++c) plan->P.mean[c] = desc->means[c], plan->P.norm[c] = desc->norms[c];
    plan->P.alpha = desc->alpha;
    plan->inDims[0] = plan->outDims[0] = desc->N;
    plan->inDims[1] = desc->H;
    plan->inDims[2] = desc->W;
    plan->inDims[3] = 1;
    plan->outDims[1] = desc->OH;
    plan->outDims[2] = desc->OW;
    plan->outDims[3] = desc->C;
    plan->bytes = srcElems * (bits / 8) + outPixels * desc->C * (half ? 2 : 4); // both inputs once (what a launch can address), the output once
    const double np = plan->single ? 1.0 : 2.0, nt = 4.0 + np;
    // per output pixel: two components, nt rows filtered for np columns, then np x np columns of nt terms, the matrix per source pixel, the blend
    plan->flops = outPixels * (2.0 * 2.0 * nt * nt * np + 2.0 * 2.0 * nt * np * np + 12.0 * np * np + (plan->single ? 0.0 : 27.0) + 6.0);
    char buf[360];
    snprintf(buf, sizeof(buf), "%s_u%d c=%d %s %s siting=%s range=%s %dx%d->%dx%d tile=%d taps=%s maxval=%d shift=%d kr=%g kb=%g kernel=%s", plan->name(), bits, desc->C,
             half ? "f16" : "f32", desc->filter == SNNHIP_YUV_TENSOR_LINEAR ? "linear" : "nearest", desc->siting == SNNHIP_SITING_LEFT ? "left" : "centre",
             desc->range == SNNHIP_RANGE_LIMITED ? "limited" : "full", desc->H, desc->W, desc->OH, desc->OW, yuv_tensor_tile(desc->C, half), plan->single ? "single" : "bilinear",
             desc->maxval, desc->shift, desc->kr, desc->kb, planar ? "yuv_tensor_planar_kernel" : "yuv_tensor_kernel");
    plan->desc = buf;
    *out = plan;
    return SNNHIP_OK;
}

int snnhip_yuv_tensor_plan_create(snnhip_ctx* ctx, const snnhip_yuv_tensor_desc* desc, snnhip_plan** out) { return yuv_tensor_plan_make(ctx, desc, out, false); }

int snnhip_yuv_tensor_planar_plan_create(snnhip_ctx* ctx, const snnhip_yuv_tensor_desc* desc, snnhip_plan** out) { return yuv_tensor_plan_make(ctx, desc, out, true); }

} // extern "C"
