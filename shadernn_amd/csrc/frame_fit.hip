// frame_fit.hip -- a plane of 8 / 16-bit samples resampled to any size between half and four times its own, each axis with its own ratio
// (include/snnhip.h: snnhip_plane_fit_plan_create / snnhip_fit_taps): what brings the r-fold frame of the luma model to the
// size a pipeline asks for (720p -> 1080p is x2, then 3/4).  The reference has no counterpart: the libyuv it vendors scales planes on the CPU with
// box / bilinear filters.
//
//   plane_fit:  E [N][H][W][C] -> E [N][OH][OW][C],  v = float(u >> shift), separable, per output coordinate eight weights over base - 3 .. base + 4
//               (the Keys cubic, stretched by min(O / I, 1) and normalised: frame_fit.h), replicate edge, q = clamp(rint(.), 0, maxval) << shift.
//
// Unlike the fixed-phase kernels next to it (frame_resample.h: r outputs per input, four taps from registers) every output coordinate has its own
// weights and a shrinking axis reaches eight taps, so the two passes meet in LDS.  A block of 256 threads owns an output tile of TH x TW pixels.
// The walk of pass 1 and the lane set-up of pass 2 are frame_fit_core.h's, shared with rgb_fit; this file has the strips and the epilogue.
//   Pass 1, vertical: the tile's input column span is cut into dword-wide strips.  A lane walks its strip down the input rows with a window of the
//     raw dwords of the last eight (four) rows, a few loads ahead of their use, and writes one filtered float row into LDS per output row; the rows'
//     bases and weights are the same for the whole block (scalar loads).  When the span has fewer strips than the block has lanes (enlarging: 45 of 256
//     for 8-bit luma at 3/2) the tile's rows are dealt to as many lane sets as fit, each walking its own chunk: the chunks' halos are read again
//     (from L1 / L2, the lines are the same), which is cheaper than three lanes in four idling through the only phase that waits on memory.
//   One barrier.
//   Pass 2, horizontal: a wave covers the tile's width, a lane the pixels of one output dword; its weights and LDS offsets sit in registers for
//     all the rows the wave takes (every fourth).  Whole dwords out; elements where the row is not dword-aligned or the dword crosses the edge.
// Rows that are not dword-aligned (odd widths) and strips that cross the plane's edge take an element path with clamped indices: no load leaves the
// plane.  An axis with O == I has base = X and weights (0, 0, 0, 1, 0, ...): the same code copies, exactly.
#include "frame_fit.h"
#include "plan_util.h"
#include "snnhip_internal.h"

namespace snnhip {
namespace {

using FitParams = FitHead; // plane_fit adds nothing to the shared head

// the strips of pass 1 (frame_fit_core.h): a strip is the dword of elements pos .. pos + NE - 1 of a row; the window keeps the raw dwords and
// converts when it filters (floats would take NE times the registers)
template <typename E, int C, bool WIDE>
struct PlaneFitStrips {
    static constexpr FitRule R = kPlaneFitRule;
    static constexpr FitGeom G{static_cast<int>(sizeof(E)), C, WIDE ? 1 : 0};
    static constexpr int ES = static_cast<int>(sizeof(E)), NE = G.ne(), K0 = G.k0(), NT = G.taps(), NR = 1, NF = NE, NW = 1;
    using Win = unsigned;
    const E* plane;
    int W, e0, shift;
    __device__ __forceinline__ int pos(int s) const { return e0 + s * NE; }
    __device__ __forceinline__ bool fast(int e) const { // the row is dword-aligned and the strip lies inside it
        return (reinterpret_cast<size_t>(plane) & 3) == 0 && (static_cast<size_t>(W) * C * ES) % 4 == 0 && e >= 0 && e + NE <= W * C;
    }
    __device__ __forceinline__ void load(int cy, int e, bool fast, unsigned* raw) const { raw[0] = fit_load_strip<E, C>(plane + static_cast<size_t>(cy) * W * C, e, W, fast); }
    __device__ __forceinline__ void enter(const unsigned* raw, unsigned* row) const { row[0] = raw[0]; }
    __device__ __forceinline__ float at(const unsigned* row, int j) const { return static_cast<float>(frame_elem<E>(row, j) >> shift); }
    __device__ __forceinline__ int off(int b) const { return (b - 3 + K0) * C - e0; }
};

template <typename E, int C, bool WIDE>
__global__ __launch_bounds__(kFitThreads) void plane_fit_kernel(FitParams P, const E* __restrict__ in, E* __restrict__ out) {
    using V = PlaneFitStrips<E, C, WIDE>;
    constexpr FitGeom G = V::G;
    constexpr FitTile T = G.tile();
    constexpr int ES = V::ES, NE = V::NE, TW = T.tw, TH = T.th(), NT = V::NT, RS = T.rowStride(), MAXS = T.maxStrips;
    constexpr int NPX = NE / C > 0 ? NE / C : 1; // pixels of an output dword (a 16-bit CbCr pixel is the whole dword)
    static_assert(TH * RS <= kFitLdsFloats && TH >= 1, "the tile's filtered rows fit the LDS");
    static_assert(C == 1 || C == 2, "one plane or interleaved CbCr");
    __shared__ float lds[kFitLdsFloats];

    const int tid = threadIdx.x;
    const FrameTile tile = frame_tile(blockIdx.x, P.tilesX, P.tilesY);
    const size_t n = tile.n;
    const int H = P.H, W = P.W, OH = P.OH, OW = P.OW;
    const int ox0 = tile.tx * TW, oy0 = tile.ty * TH;
    const int tcols = min(TW, OW - ox0), trows = min(TH, OH - oy0);
    const E* plane = in + n * H * W * C;

    // the tile's input column span as dword strips: elements e0 .. e0 + S * NE - 1 of a row
    const int e0 = G.first(P.bx[ox0]);
    const int S = min(G.strips(e0, P.bx[ox0 + tcols - 1]), MAXS); // (the plan checked every tile against MAXS)

    const V v{plane, W, e0, P.shift};
    fit_vertical_pass(v, P, lds, RS, S, oy0, trows, tid);
    __syncthreads();

    // ---- pass 2: quantise and pack.  Whole dwords out; elements where the row is not dword-aligned or the dword crosses the edge.
    const int g = tid & 63; // the lane's dword of an output row of the tile
    if (g * NPX >= tcols) return;
    const FitLane<NPX, NT> L = fit_lane<NPX>(v, P, g, ox0, tcols);
    const int valid = L.valid * C; // elements of the lane's dword inside the plane
    E* oplane = out + n * OH * OW * C;
    const bool whole = valid == NE && (reinterpret_cast<size_t>(oplane) & 3) == 0 && (static_cast<size_t>(OW) * C * ES) % 4 == 0;
    for (int t = tid >> 6; t < trows; t += kFitWaves) {
        const float* src = lds + t * RS;
        unsigned q[NE];
#pragma unroll
        for (int j = 0; j < NE; ++j) {
            const int p = j / C, c = j % C;
            float acc = L.w[p][0] * src[fit_skew(L.off[p] + c)];
#pragma unroll
            for (int k = 1; k < NT; ++k) acc += L.w[p][k] * src[fit_skew(L.off[p] + k * C + c)];
            q[j] = quantize_frame(acc, P.maxval) << P.shift;
        }
        E* dst = oplane + (static_cast<size_t>(oy0 + t) * OW + ox0) * C + static_cast<size_t>(g) * NE;
        if (whole) {
            unsigned word = 0u;
#pragma unroll
            for (int j = 0; j < NE; ++j) word |= q[j] << (8 * ES * j);
            store_words<1>(dst, &word);
        } else {
#pragma unroll
            for (int j = 0; j < NE; ++j)
                if (j < valid) dst[j] = static_cast<E>(q[j]);
        }
    }
}

struct PlaneFitPlan : snnhip_plan {
    snnhip_plane_fit_desc d;
    FitParams P;
    bool wide = false;

    template <typename E>
    void launch(const snnhip_tensor* in, snnhip_tensor* out) {
        const dim3 grid(static_cast<unsigned>(P.N) * static_cast<unsigned>(P.tilesX) * static_cast<unsigned>(P.tilesY));
        const E* src = reinterpret_cast<const E*>(in->data);
        E* dst = reinterpret_cast<E*>(out->data);
        auto go = [&](auto Cc, auto Wd) {
            SNNHIP_LAUNCH((plane_fit_kernel<E, decltype(Cc)::value, decltype(Wd)::value>), grid, dim3(kFitThreads), 0, ctx->stream, P, src, dst);
        };
        if (d.C == 1) {
            if (wide) go(std::integral_constant<int, 1>{}, std::true_type{});
            else go(std::integral_constant<int, 1>{}, std::false_type{});
        } else {
            if (wide) go(std::integral_constant<int, 2>{}, std::true_type{});
            else go(std::integral_constant<int, 2>{}, std::false_type{});
        }
    }

    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        SNNHIP_REQUIRE(nIn == 1, "plane_fit: expects 1 input, got %d", nIn);
        SNNHIP_REQUIRE(in[0]->dtype == d.dtype && out->dtype == d.dtype, "plane_fit: both tensors must have dtype %d, got %d and %d", d.dtype, in[0]->dtype, out->dtype);
        SNNHIP_REQUIRE(dims_match(in[0], d.N, d.H, d.W, d.C), "plane_fit: the input plane is %dx%dx%dx%d, the plan was built for %dx%dx%dx%d", in[0]->n, in[0]->h, in[0]->w,
                       in[0]->c, d.N, d.H, d.W, d.C);
        SNNHIP_REQUIRE(dims_match(out, d.N, d.OH, d.OW, d.C), "plane_fit: the output is %dx%dx%dx%d, the plan was built for %dx%dx%dx%d", out->n, out->h, out->w, out->c, d.N,
                       d.OH, d.OW, d.C);
        if (d.dtype == SNNHIP_U8) launch<unsigned char>(in[0], out);
        else launch<unsigned short>(in[0], out);
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }
};

} // namespace
} // namespace snnhip

using namespace snnhip;

extern "C" {

int snnhip_fit_taps(int in, int out, int siting, float* weights, int* base, int capacity) {
    return fill_fit_taps(kPlaneFitRule, "fit_taps", in, out, siting, weights, base, capacity);
}

int snnhip_plane_fit_plan_create(snnhip_ctx* ctx, const snnhip_plane_fit_desc* desc, snnhip_plan** out) {
    SNNHIP_REQUIRE(ctx && desc && out, "plane_fit_plan_create: null argument");
    SNNHIP_REQUIRE(desc->N > 0 && desc->H > 0 && desc->W > 0 && desc->OH > 0 && desc->OW > 0, "plane_fit desc: bad dims %dx%dx%d -> %dx%d", desc->N, desc->H, desc->W,
                   desc->OH, desc->OW);
    SNNHIP_REQUIRE(desc->C == 1 || desc->C == 2, "plane_fit desc: %d channels (1: a luma plane or one plane of a planar format, 2: interleaved CbCr)", desc->C);
    SNNHIP_REQUIRE(2ll * desc->OH >= desc->H && desc->OH <= 4ll * desc->H, "plane_fit desc: the vertical axis goes from %d to %d rows, a ratio outside [1/2, 4]", desc->H,
                   desc->OH);
    SNNHIP_REQUIRE(2ll * desc->OW >= desc->W && desc->OW <= 4ll * desc->W, "plane_fit desc: the horizontal axis goes from %d to %d columns, a ratio outside [1/2, 4]",
                   desc->W, desc->OW);
    int bits = 0;
    const int fmt = check_sample_format("plane_fit desc", "planes", desc->dtype, desc->siting, desc->shift, desc->maxval, &bits);
    if (fmt != SNNHIP_OK) return fmt;
    const bool wide = desc->OH < desc->H || desc->OW < desc->W;
    const FitGeom g{bits / 8, desc->C, wide ? 1 : 0};
    const FitTile tile = g.tile();
    const double inElems = static_cast<double>(desc->N) * desc->H * desc->W * desc->C;
    const double outElems = static_cast<double>(desc->N) * desc->OH * desc->OW * desc->C;
    SNNHIP_REQUIRE(inElems < 9.0e15 && outElems < 9.0e15 && static_cast<double>(desc->W) * desc->C < 1.0e9, "plane_fit desc: %dx%dx%d -> %dx%d is too large", desc->N, desc->H,
                   desc->W, desc->OH, desc->OW);
    FitAxes axes;
    int rc = axes.build("plane_fit", snnhip_fit_taps, kFitTaps, g, desc->N, desc->H, desc->W, desc->OH, desc->OW, desc->siting);
    if (rc != SNNHIP_OK) return rc;
    auto* plan = new PlaneFitPlan();
    plan->ctx = ctx;
    plan->dtype = desc->dtype;
    plan->rawInput = desc->dtype;
    plan->rawOutput = desc->dtype;
    plan->d = *desc;
    plan->wide = wide;
    rc = axes.upload(plan, &plan->P, desc->shift, desc->maxval);
    if (rc != SNNHIP_OK) {
        delete plan;
        return rc;
    }
    plan->inDims[0] = plan->outDims[0] = desc->N;
    plan->inDims[1] = desc->H;
    plan->inDims[2] = desc->W;
    plan->outDims[1] = desc->OH;
    plan->outDims[2] = desc->OW;
    plan->inDims[3] = plan->outDims[3] = desc->C;
    plan->bytes = (inElems + outElems) * (bits / 8); // the input once, the output once
    const int nt = g.taps();
    plan->flops = 2.0 * nt * (outElems + static_cast<double>(desc->N) * desc->OH * desc->W * desc->C); // both passes
    char buf[280];
    snprintf(buf, sizeof(buf), "plane_fit_u%d c=%d %dx%d->%dx%d siting=%s tile=%dx%d taps=%d lds=%d maxval=%d shift=%d kernel=plane_fit_kernel", bits, desc->C, desc->H,
             desc->W, desc->OH, desc->OW, desc->siting == SNNHIP_SITING_LEFT ? "left" : "centre", tile.th(), tile.tw, nt, static_cast<int>(kFitLdsFloats * sizeof(float)),
             desc->maxval, desc->shift);
    plan->desc = buf;
    *out = plan;
    return SNNHIP_OK;
}

} // extern "C"
