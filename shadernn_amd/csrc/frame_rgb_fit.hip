// frame_rgb_fit.hip -- packed RGB at any output size behind a luma-only model (include/snnhip.h: snnhip_rgb_fit_plan_create / snnhip_rgb_fit_taps;
// DESIGN.md section 4.24): the luma frame already at the output size and the ORIGINAL low-resolution chroma source in, RGB / RGBA out, in one
// launch.  The reference has no counterpart: the libyuv it vendors scales and converts on the CPU.
//
//   rgb_fit:  Yfit E [N][OH][OW][1] + the chroma source -> E [N][OH][OW][C], C = 3 | 4.  The source is CbCr E [N][H][W][2] (NV12 / P010), two planes
//             E [2N][H][W][1] (I420 / I010) or the low-resolution colour frame U8 [N][H][W][C]; it is enlarged 1- to 8-fold, each axis with its own
//             ratio, four normalised Keys weights per output coordinate (frame_rgb_fit.h), replicate edge, vertical then horizontal.  The matrix and
//             the quantiser are yuv_rgb's for the video sources and ycc_merge's for the colour frame.
//
// The fixed-phase RGB kernels (frame_yuv_rgb.hip, frame_colour.hip) keep r or 2r phases in registers; a base per output coordinate would turn their
// register windows into dynamically indexed arrays, that is, scratch.  So this kernel has plane_fit's shape (frame_fit.hip) and shares its walk
// (frame_fit_core.h: pass 1, the lane set-up of pass 2): the two passes meet in LDS, and a block of 256 threads owns an output tile of TH x TW pixels.
//   Pass 1, vertical: the tile's source column span is cut into strips of SP pixels -- a dword of CbCr, a dword of each plane, four RGB(A) pixels --
//     one lane per strip.  A lane walks its strip down the source rows with a window of the last four rows as float pairs, (Cb - Coff, Cr - Coff) or
//     (dB, dR), converted once when a row enters (an enlarged source row serves several output rows); raw loads run a few rows ahead of their use.
//     It writes one filtered row of interleaved pairs into LDS per output row; the rows' bases and weights are the same for the whole block.  When
//     the span has fewer strips than the block has lanes, the tile's rows are dealt to as many lane sets as fit, as in plane_fit.
//   One barrier.
//   Pass 2, horizontal: a wave covers the tile's width, a lane the pixels of one dword of Yfit; its four weights per pixel and its LDS offsets sit
//     in registers for all the rows the wave takes (every fourth).  Per row: the taps from LDS, the Yfit dword from memory, the matrix, the
//     quantiser, C dwords out; elements where a row is not dword-aligned or the dword crosses the edge.
// Rows that are not dword-aligned, strips that cross the source's edge and everything outside it take an element path with clamped indices: no
// load leaves a tensor.  LDS rows keep plane_fit's skew (one float every 32); a pair of floats is then not always 8-byte aligned and is read as two
// dwords.
#include "frame_rgb_fit.h"
#include "plan_util.h"
#include "snnhip_internal.h"

namespace snnhip {
namespace {

struct RgbFitParams : FitHead { // H, W: the chroma source
    unsigned alpha;   // maxval << shift (video sources)
    YuvRgbCoeffs m;   // video sources
    float kr, kg, kb; // the RGB source
};

// the strips of pass 1 (frame_fit_core.h): a strip is SP source pixels from pixel pos on -- a dword of CbCr, a dword of each plane, four RGB(A)
// pixels; the window keeps float pairs, converted once when a row enters (an enlarged source row serves several output rows)
template <typename E, int SRC, int CO>
struct RgbFitStrips {
    static constexpr FitRule R = kRgbFitRule;
    static constexpr int ES = static_cast<int>(sizeof(E)), NE = 4 / ES, BITS = 8 * ES;
    static constexpr RgbFitGeom G{ES, SRC};
    static constexpr int K0 = R.k0, NT = R.nk;
    static constexpr int SP = G.sp();                                                                   // source pixels of a strip
    static constexpr int NF = 2 * SP, NW = NF;                                                          // floats of a strip in a filtered row
    static constexpr int NR = SRC == SNNHIP_RGB_FIT_CBCR ? 1 : SRC == SNNHIP_RGB_FIT_PLANAR ? 2 : CO; // raw dwords of a strip in a source row
    static_assert(SRC != SNNHIP_RGB_FIT_RGB || ES == 1, "colour frames are 8-bit");
    static_assert(SRC != SNNHIP_RGB_FIT_CBCR || NF == NE, "a CbCr strip is one dword");
    using Win = float;
    const RgbFitParams& P;
    const E* img; // image n of the source: its CbCr plane, its Cb plane (Cr follows planeElems behind it) or its colour frame
    size_t planeElems;
    int W, px0;
    bool rowsAligned; // every row of the image starts on a dword (one decision for the block)

    __device__ __forceinline__ RgbFitStrips(const RgbFitParams& P_, const E* img_, size_t planeElems_, int px0_) : P(P_), img(img_), planeElems(planeElems_), W(P_.W), px0(px0_) {
        if constexpr (SRC == SNNHIP_RGB_FIT_CBCR) rowsAligned = (reinterpret_cast<size_t>(img) & 3) == 0 && (static_cast<size_t>(W) * 2 * ES) % 4 == 0;
        else if constexpr (SRC == SNNHIP_RGB_FIT_PLANAR)
            rowsAligned = ((reinterpret_cast<size_t>(img) | reinterpret_cast<size_t>(img + planeElems)) & 3) == 0 && (static_cast<size_t>(W) * ES) % 4 == 0;
        else rowsAligned = (reinterpret_cast<size_t>(img) & 3) == 0 && (static_cast<size_t>(W) * CO) % 4 == 0;
    }
    __device__ __forceinline__ int pos(int s) const { return px0 + s * SP; }
    // (px is a multiple of SP, so a strip inside the row starts on a dword)
    __device__ __forceinline__ bool fast(int px) const { return rowsAligned && px >= 0 && px + SP <= W; }
    // the raw dwords of source pixels px .. px + SP - 1 of row cy; unless `fast`, by elements, the pixel index clamped to [0, W - 1]
    __device__ __forceinline__ void load(int cy, int px, bool fast, unsigned* raw) const {
        if constexpr (SRC == SNNHIP_RGB_FIT_CBCR) {
            raw[0] = fit_load_strip<E, 2>(img + static_cast<size_t>(cy) * W * 2, px * 2, W, fast);
        } else if constexpr (SRC == SNNHIP_RGB_FIT_PLANAR) {
#pragma unroll
            for (int c = 0; c < 2; ++c) raw[c] = fit_load_strip<E, 1>(img + c * planeElems + static_cast<size_t>(cy) * W, px, W, fast);
        } else {
            const E* row = img + static_cast<size_t>(cy) * W * CO;
            if (fast) {
                load_words<CO>(row + static_cast<size_t>(px) * CO, raw);
            } else {
#pragma unroll
                for (int k = 0; k < CO; ++k) raw[k] = 0u;
#pragma unroll
                for (int i = 0; i < 4 * CO; ++i) {
                    const int p = min(max(px + i / CO, 0), W - 1);
                    raw[i >> 2] |= static_cast<unsigned>(row[static_cast<size_t>(p) * CO + i % CO]) << (8 * (i & 3));
                }
            }
        }
    }
    // a strip's raw dwords as the float pairs that are filtered: (Cb - Coff, Cr - Coff), exact in fp32, or (dB, dR) around the unquantised luma
    __device__ __forceinline__ void enter(const unsigned* raw, float* f) const {
        if constexpr (SRC == SNNHIP_RGB_FIT_CBCR) {
#pragma unroll
            for (int j = 0; j < NF; ++j) f[j] = static_cast<float>(frame_elem<E>(raw, j) >> P.shift) - P.m.coff;
        } else if constexpr (SRC == SNNHIP_RGB_FIT_PLANAR) {
#pragma unroll
            for (int p = 0; p < SP; ++p) {
                f[2 * p] = static_cast<float>(frame_elem<E>(raw, p) >> P.shift) - P.m.coff;
                f[2 * p + 1] = static_cast<float>(frame_elem<E>(raw + 1, p) >> P.shift) - P.m.coff;
            }
        } else {
#pragma unroll
            for (int p = 0; p < SP; ++p) {
                const float r = static_cast<float>(frame_elem<E>(raw, p * CO)), g = static_cast<float>(frame_elem<E>(raw, p * CO + 1)),
                            b = static_cast<float>(frame_elem<E>(raw, p * CO + 2));
                const float yl = luma_f32(r, g, b, P.kr, P.kg, P.kb);
                f[2 * p] = b - yl;
                f[2 * p + 1] = r - yl;
            }
        }
    }
    __device__ __forceinline__ float at(const float* row, int j) const { return row[j]; }
    __device__ __forceinline__ int off(int b) const { return (b - 1 - px0) * 2; }
};

template <typename E, int SRC, int CO>
__global__ __launch_bounds__(kFitThreads) void rgb_fit_kernel(RgbFitParams P, const E* __restrict__ yfit, const E* __restrict__ src, E* __restrict__ out) {
    using V = RgbFitStrips<E, SRC, CO>;
    constexpr RgbFitGeom G = V::G;
    constexpr FitTile T = G.tile();
    constexpr int ES = V::ES, NE = V::NE, BITS = V::BITS, NT = V::NT;
    constexpr int NPX = G.npx(), TW = T.tw, TH = T.th(), RS = T.rowStride(), MAXS = T.maxStrips;
    static_assert(TH * RS <= kFitLdsFloats && TH >= 1, "the tile's filtered rows fit the LDS");
    static_assert(NPX == NE, "a lane owns one dword of Yfit");
    __shared__ float lds[kFitLdsFloats];

    const int tid = threadIdx.x;
    const FrameTile tile = frame_tile(blockIdx.x, P.tilesX, P.tilesY);
    const size_t n = tile.n;
    const int H = P.H, W = P.W, OH = P.OH, OW = P.OW;
    const int ox0 = tile.tx * TW, oy0 = tile.ty * TH;
    const int tcols = min(TW, OW - ox0), trows = min(TH, OH - oy0);
    const size_t planeElems = static_cast<size_t>(H) * W;
    const E* img = src + n * planeElems * (SRC == SNNHIP_RGB_FIT_RGB ? CO : 2);

    // the tile's source column span as strips: pixels px0 .. px0 + S * SP - 1
    const int px0 = G.first(P.bx[ox0]);
    const int S = min(G.strips(px0, P.bx[ox0 + tcols - 1]), MAXS); // (the plan checked every tile against MAXS)

    const V v(P, img, planeElems, px0);
    fit_vertical_pass(v, P, lds, RS, S, oy0, trows, tid);
    __syncthreads();

    // ---- pass 2.  Per row: the taps from LDS, the Yfit dword from memory, the matrix, the quantiser, C dwords out
    const int g = tid & 63; // the lane's dword of a row of Yfit
    if (g * NPX >= tcols) return;
    const FitLane<NPX, NT> F = fit_lane<NPX>(v, P, g, ox0, tcols);
    int ax[NPX]; // the source column whose alpha an output column copies (colour frames with C = 4)
#pragma unroll
    for (int p = 0; p < NPX; ++p) ax[p] = static_cast<int>((2ll * F.X[p] + 1) * W / (2ll * OW));
    const int valid = F.valid; // pixels of the lane's dword inside the frame
    const E* yimg = yfit + n * OH * OW;
    E* oimg = out + n * OH * OW * CO;
    const bool whole = valid == NPX && ((reinterpret_cast<size_t>(yimg) | reinterpret_cast<size_t>(oimg)) & 3) == 0 && (static_cast<size_t>(OW) * ES) % 4 == 0 &&
                       (static_cast<size_t>(OW) * CO * ES) % 4 == 0;
    for (int t = tid >> 6; t < trows; t += kFitWaves) {
        const float* row = lds + t * RS;
        const size_t pix = static_cast<size_t>(oy0 + t) * OW + ox0 + static_cast<size_t>(g) * NPX;
        unsigned u = 0u;
        if (whole) {
            load_words<1>(yimg + pix, &u);
        } else {
#pragma unroll
            for (int j = 0; j < NPX; ++j)
                if (j < valid) u |= static_cast<unsigned>(yimg[pix + j]) << (BITS * j);
        }
        const E* arow = img; // (read for colour frames with C = 4 only)
        if constexpr (SRC == SNNHIP_RGB_FIT_RGB && CO == 4) arow = img + static_cast<size_t>((2ll * (oy0 + t) + 1) * H / (2ll * OH)) * W * CO;
        unsigned word[CO];
#pragma unroll
        for (int k = 0; k < CO; ++k) word[k] = 0u;
#pragma unroll
        for (int p = 0; p < NPX; ++p) {
            float c0 = F.w[p][0] * row[fit_skew(F.off[p])], c1 = F.w[p][0] * row[fit_skew(F.off[p] + 1)];
#pragma unroll
            for (int k = 1; k < NT; ++k) {
                c0 += F.w[p][k] * row[fit_skew(F.off[p] + 2 * k)];
                c1 += F.w[p][k] * row[fit_skew(F.off[p] + 2 * k + 1)];
            }
            const float yv = static_cast<float>(frame_elem<E>(&u, p) >> P.shift);
            unsigned e[4];
            if constexpr (SRC == SNNHIP_RGB_FIT_RGB) { // c0 = dB~, c1 = dR~
                e[0] = quantize_frame(yv + c1, P.maxval);
                e[1] = quantize_frame(yv - (P.kr * c1 + P.kb * c0) / P.kg, P.maxval);
                e[2] = quantize_frame(yv + c0, P.maxval);
                e[3] = CO == 4 ? static_cast<unsigned>(arow[static_cast<size_t>(ax[p]) * CO + 3]) : 0u;
            } else { // c0 = Cb~ - Coff, c1 = Cr~ - Coff
                const float yl = P.m.cy * (yv - P.m.yoff);
                e[0] = quantize_frame(yl + P.m.crv * c1, P.maxval) << P.shift;
                e[1] = quantize_frame(yl - (P.m.cgv * c1 + P.m.cgu * c0), P.maxval) << P.shift;
                e[2] = quantize_frame(yl + P.m.cbu * c0, P.maxval) << P.shift;
                e[3] = P.alpha;
            }
#pragma unroll
            for (int c = 0; c < CO; ++c) {
                const int i = p * CO + c;
                word[i / NE] |= e[c] << (BITS * (i % NE));
            }
        }
        E* dst = oimg + pix * CO;
        if (whole) {
            store_words<CO>(dst, word);
        } else {
#pragma unroll
            for (int i = 0; i < NPX * CO; ++i)
                if (i < valid * CO) dst[i] = static_cast<E>(frame_elem<E>(word, i));
        }
    }
}

const char* source_name(int source) { return source == SNNHIP_RGB_FIT_CBCR ? "cbcr" : source == SNNHIP_RGB_FIT_PLANAR ? "planar" : "rgb"; }

struct RgbFitPlan : snnhip_plan {
    snnhip_rgb_fit_desc d; // (for the RGB source: dtype U8, maxval 255, shift 0, centre as the kernel uses them)
    RgbFitParams P;

    template <typename E, int SRC>
    void launch(const snnhip_tensor* y, const snnhip_tensor* c, snnhip_tensor* out) {
        const dim3 grid(static_cast<unsigned>(P.N) * static_cast<unsigned>(P.tilesX) * static_cast<unsigned>(P.tilesY));
        const E* ysrc = reinterpret_cast<const E*>(y->data);
        const E* csrc = reinterpret_cast<const E*>(c->data);
        E* dst = reinterpret_cast<E*>(out->data);
        if (d.C == 3) SNNHIP_LAUNCH((rgb_fit_kernel<E, SRC, 3>), grid, dim3(kFitThreads), 0, ctx->stream, P, ysrc, csrc, dst);
        else SNNHIP_LAUNCH((rgb_fit_kernel<E, SRC, 4>), grid, dim3(kFitThreads), 0, ctx->stream, P, ysrc, csrc, dst);
    }

    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        SNNHIP_REQUIRE(nIn == 2, "rgb_fit: expects 2 inputs (Yfit, the chroma source), got %d", nIn);
        SNNHIP_REQUIRE(in[0]->dtype == d.dtype && in[1]->dtype == d.dtype && out->dtype == d.dtype, "rgb_fit: every tensor must have dtype %d, got %d, %d and %d", d.dtype,
                       in[0]->dtype, in[1]->dtype, out->dtype);
        const int sn = d.source == SNNHIP_RGB_FIT_PLANAR ? 2 * d.N : d.N;
        const int sc = d.source == SNNHIP_RGB_FIT_CBCR ? 2 : d.source == SNNHIP_RGB_FIT_PLANAR ? 1 : d.C;
        SNNHIP_REQUIRE(dims_match(in[1], sn, d.H, d.W, sc), "rgb_fit: the chroma source is %dx%dx%dx%d, the plan (src=%s) was built for %dx%dx%dx%d", in[1]->n, in[1]->h,
                       in[1]->w, in[1]->c, source_name(d.source), sn, d.H, d.W, sc);
        SNNHIP_REQUIRE(dims_match(in[0], d.N, d.OH, d.OW, 1), "rgb_fit: Yfit is %dx%dx%dx%d, the plan was built for %dx%dx%dx1 (the luma frame at the output size)", in[0]->n,
                       in[0]->h, in[0]->w, in[0]->c, d.N, d.OH, d.OW);
        SNNHIP_REQUIRE(dims_match(out, d.N, d.OH, d.OW, d.C), "rgb_fit: the output is %dx%dx%dx%d, the plan was built for %dx%dx%dx%d", out->n, out->h, out->w, out->c, d.N,
                       d.OH, d.OW, d.C);
        if (d.source == SNNHIP_RGB_FIT_RGB) launch<unsigned char, SNNHIP_RGB_FIT_RGB>(in[0], in[1], out);
        else if (d.source == SNNHIP_RGB_FIT_CBCR) {
            if (d.dtype == SNNHIP_U8) launch<unsigned char, SNNHIP_RGB_FIT_CBCR>(in[0], in[1], out);
            else launch<unsigned short, SNNHIP_RGB_FIT_CBCR>(in[0], in[1], out);
        } else {
            if (d.dtype == SNNHIP_U8) launch<unsigned char, SNNHIP_RGB_FIT_PLANAR>(in[0], in[1], out);
            else launch<unsigned short, SNNHIP_RGB_FIT_PLANAR>(in[0], in[1], out);
        }
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }
};

} // namespace
} // namespace snnhip

using namespace snnhip;

extern "C" {

int snnhip_rgb_fit_taps(int in, int out, int siting, float* weights, int* base, int capacity) {
    return fill_fit_taps(kRgbFitRule, "rgb_fit_taps", in, out, siting, weights, base, capacity);
}

int snnhip_rgb_fit_plan_create(snnhip_ctx* ctx, const snnhip_rgb_fit_desc* desc, snnhip_plan** out) {
    SNNHIP_REQUIRE(ctx && desc && out, "rgb_fit_plan_create: null argument");
    SNNHIP_REQUIRE(desc->N > 0 && desc->H > 0 && desc->W > 0 && desc->OH > 0 && desc->OW > 0, "rgb_fit desc: bad dims %dx%dx%d -> %dx%d", desc->N, desc->H, desc->W, desc->OH,
                   desc->OW);
    SNNHIP_REQUIRE(desc->C == 3 || desc->C == 4, "rgb_fit desc: %d channels (3: RGB, 4: RGBA)", desc->C);
    SNNHIP_REQUIRE(desc->source == SNNHIP_RGB_FIT_CBCR || desc->source == SNNHIP_RGB_FIT_PLANAR || desc->source == SNNHIP_RGB_FIT_RGB,
                   "rgb_fit desc: source %d (SNNHIP_RGB_FIT_CBCR, SNNHIP_RGB_FIT_PLANAR or SNNHIP_RGB_FIT_RGB)", desc->source);
    SNNHIP_REQUIRE(desc->OH >= desc->H && desc->OH <= 8ll * desc->H, "rgb_fit desc: the vertical axis goes from %d to %d rows, a ratio outside [1, 8]", desc->H, desc->OH);
    SNNHIP_REQUIRE(desc->OW >= desc->W && desc->OW <= 8ll * desc->W, "rgb_fit desc: the horizontal axis goes from %d to %d columns, a ratio outside [1, 8]", desc->W,
                   desc->OW);
    const bool video = desc->source != SNNHIP_RGB_FIT_RGB;
    snnhip_rgb_fit_desc d = *desc;
    int bits = 8;
    if (video) {
        const int fmt = check_sample_format("rgb_fit desc", "frames", desc->dtype, desc->siting, desc->shift, desc->maxval, &bits);
        if (fmt != SNNHIP_OK) return fmt;
        SNNHIP_REQUIRE(desc->range == SNNHIP_RANGE_LIMITED || desc->range == SNNHIP_RANGE_FULL, "rgb_fit desc: range %d (SNNHIP_RANGE_LIMITED or SNNHIP_RANGE_FULL)", desc->range);
        SNNHIP_REQUIRE((desc->maxval + 1) % 256 == 0, "rgb_fit desc: maxval %d: maxval + 1 must be a multiple of 256 (the offsets 16k, 128k of the matrix are integers)",
                       desc->maxval);
    } else {
        SNNHIP_REQUIRE(desc->dtype == SNNHIP_U8, "rgb_fit desc: dtype %d with the RGB source (colour frames are SNNHIP_U8)", desc->dtype);
        d.maxval = 255, d.shift = 0, d.siting = SNNHIP_SITING_CENTRE, d.range = SNNHIP_RANGE_FULL;
    }
    SNNHIP_REQUIRE(matrix_ok(desc->kr, desc->kb), "rgb_fit desc: kr = %g, kb = %g (0 < kr, 0 < kb, kr + kb < 1)", desc->kr, desc->kb);
    const RgbFitGeom g{bits / 8, d.source};
    const FitTile tile = g.tile();
    const int sc = d.source == SNNHIP_RGB_FIT_RGB ? d.C : 2;
    const double srcElems = static_cast<double>(d.N) * d.H * d.W * sc;
    const double outPixels = static_cast<double>(d.N) * d.OH * d.OW;
    SNNHIP_REQUIRE(srcElems < 9.0e15 && outPixels * d.C < 9.0e15 && static_cast<double>(d.W) * sc < 1.0e9 && 2.0 * d.N < 2147483648.0,
                   "rgb_fit desc: %dx%dx%d -> %dx%d is too large", d.N, d.H, d.W, d.OH, d.OW);
    FitAxes axes;
    int rc = axes.build("rgb_fit", snnhip_rgb_fit_taps, kRgbFitTaps, g, d.N, d.H, d.W, d.OH, d.OW, d.siting);
    if (rc != SNNHIP_OK) return rc;
    // what the kernel relies on beyond the core's checks: bases stay within one pixel of the source
    const std::vector<int>&by = axes.by, &bx = axes.bx;
    SNNHIP_REQUIRE(bx[0] >= -1 && bx[d.OW - 1] < d.W && by[0] >= -1 && by[d.OH - 1] < d.H, "rgb_fit: bases %d..%d / %d..%d leave the %dx%d source", by[0], by[d.OH - 1], bx[0],
                   bx[d.OW - 1], d.H, d.W);
    auto* plan = new RgbFitPlan();
    plan->ctx = ctx;
    plan->numInputs = 2;
    plan->dtype = d.dtype; // (input 1, the chroma source, is checked against this; input 0 against rawInput)
    plan->rawInput = d.dtype;
    plan->rawOutput = d.dtype;
    plan->d = d;
    plan->P = RgbFitParams{};
    rc = axes.upload(plan, &plan->P, d.shift, d.maxval);
    if (rc != SNNHIP_OK) {
        delete plan;
        return rc;
    }
    plan->P.alpha = static_cast<unsigned>(d.maxval) << d.shift;
    if (video) plan->P.m = yuv_rgb_coeffs(d.maxval, d.range, d.kr, d.kb);
    plan->P.kr = d.kr;
    plan->P.kg = static_cast<float>(1.0 - static_cast<double>(d.kr) - static_cast<double>(d.kb)); // as rgb_luma and ycc_merge form it
    plan->P.kb = d.kb;
    plan->inDims[0] = plan->outDims[0] = d.N;
    plan->inDims[1] = plan->outDims[1] = d.OH;
    plan->inDims[2] = plan->outDims[2] = d.OW;
    plan->inDims[3] = 1;
    plan->outDims[3] = d.C;
    plan->bytes = (outPixels + srcElems + outPixels * d.C) * (bits / 8); // Yfit, the chroma source and the output: once each
    // two components, four taps per pass (the vertical pass over the source's columns), the matrix
    plan->flops = 2.0 * 2.0 * kRgbFitTaps * (outPixels + static_cast<double>(d.N) * d.OH * d.W) + 12.0 * outPixels;
    char buf[320];
    snprintf(buf, sizeof(buf), "rgb_fit_u%d src=%s c=%d %dx%d->%dx%d siting=%s range=%s tile=%dx%d taps=%d lds=%d maxval=%d shift=%d kr=%g kb=%g kernel=rgb_fit_kernel", bits,
             source_name(d.source), d.C, d.H, d.W, d.OH, d.OW, d.siting == SNNHIP_SITING_LEFT ? "left" : "centre", d.range == SNNHIP_RANGE_LIMITED ? "limited" : "full", tile.th(),
             tile.tw, kRgbFitTaps, static_cast<int>(kFitLdsFloats * sizeof(float)), d.maxval, d.shift, d.kr, d.kb);
    plan->desc = buf;
    *out = plan;
    return SNNHIP_OK;
}

} // extern "C"
