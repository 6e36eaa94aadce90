// frame_chroma.hip -- the chroma plane of a 4:2:0 video frame (NV12 / P010: interleaved CbCr, C = 2; I420 / yuv420p10le: one plane, C = 1) upsampled
// r-fold beside a luma-only model (include/snnhip.h: snnhip_chroma_up_plan_create / snnhip_bicubic_taps_sited).  The reference
// has no counterpart: core/inc/snn/color.h only names YUV layouts, and the libyuv it vendors scales planes with box / bilinear filters on the CPU.
//
//   chroma_up:  E [N][H][W][C] -> E [N][rH][rW][C],  v = float(u >> shift), separable Keys cubic (a = -0.5), horizontal then vertical, replicate edge,
//               q = clamp(rint(.), 0, maxval) << shift.  The vertical axis uses aligned sample centres, the horizontal axis the desc's siting.
//
// The kernel is HBM-bound and small (1 MB in, 4 MB out for a 1080p -> 4K NV12 frame), so it keeps nothing but loads and stores on its critical path:
// no LDS, no barrier.  One lane owns a few whole input pixels of a row (ChromaGeom::IN = 4, 8 or 16 bytes, one aligned load) and the R * IN bytes under
// them in each of R output rows (16-byte stores).  The two apron pixels either side are one more aligned load each (2, 4 or 8 bytes; they hit the lines
// the neighbouring lanes load).  A wave is 64 lanes side by side and marches down kChromaRows input rows: it filters kChromaRows + 4 rows horizontally
// in registers -- an interior lane issues all 3 * (kChromaRows + 4) loads before it waits for the first -- and forms every output row from five of them.  The per-phase base offset
// (-1 or 0) is folded into the tap table on the host: a phase is five weights over x - 2 .. x + 2 with a zero in the place it does not read, so that
// every register index is a compile-time constant (a term 0 * v adds exactly nothing).  Rows whose address is not aligned (odd widths), lanes that
// straddle the right edge and aprons outside the plane take an element path with clamped indices.
#include "frame_chroma.h"
#include "plan_util.h"
#include "snnhip_internal.h"

namespace snnhip {
namespace {

struct ChromaParams {
    int N, H, W; // the INPUT plane
    int tilesX, tilesY;
    int shift;
    float maxval;
    float wh[4][5]; // [phase][offset -2 .. 2] along a row (the desc's siting); rows r.. unused
    float wv[4][5]; // ... along a column (aligned centres)
};

// BYTES (2, 4, 8 or 16) from an address aligned to BYTES, as dwords
template <int BYTES>
__device__ __forceinline__ void chroma_load(const void* p, unsigned* w) {
    if constexpr (BYTES == 16) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
    } else if constexpr (BYTES == 8) {
        const uint2 q = *reinterpret_cast<const uint2*>(p);
        w[0] = q.x, w[1] = q.y;
    } else if constexpr (BYTES == 4) {
        w[0] = *reinterpret_cast<const unsigned*>(p);
    } else {
        w[0] = *reinterpret_cast<const unsigned short*>(p);
    }
}

// v[b * C + c] = value of input pixel (x0 - 2 + b, channel c) of the row at `row`, indices clamped to [0, W - 1]; x0 < W
template <int R, int C, typename E>
__device__ __forceinline__ void chroma_load_row(const E* __restrict__ row, int x0, int W, int shift, float* v) {
    using G = ChromaGeom<R, C, E>;
    constexpr int AP = G::AE * G::ES; // apron bytes on one side
    const bool aligned = (reinterpret_cast<size_t>(row) & (G::IN - 1)) == 0;
    if (aligned && x0 + G::PX <= W) {
        unsigned w[G::IN / 4];
        chroma_load<G::IN>(row + static_cast<size_t>(x0) * C, w);
#pragma unroll
        for (int e = 0; e < G::NE; ++e) v[G::AE + e] = static_cast<float>(frame_elem<E>(w, e) >> shift);
    } else {
#pragma unroll
        for (int e = 0; e < G::NE; ++e) {
            const int px = min(x0 + e / C, W - 1);
            v[G::AE + e] = static_cast<float>(static_cast<unsigned>(row[static_cast<size_t>(px) * C + e % C]) >> shift);
        }
    }
    if (aligned && x0 >= 2) {
        unsigned w[(AP + 3) / 4];
        chroma_load<AP>(row + static_cast<size_t>(x0 - 2) * C, w);
#pragma unroll
        for (int e = 0; e < G::AE; ++e) v[e] = static_cast<float>(frame_elem<E>(w, e) >> shift);
    } else {
#pragma unroll
        for (int e = 0; e < G::AE; ++e) {
            const int px = max(x0 - 2 + e / C, 0);
            v[e] = static_cast<float>(static_cast<unsigned>(row[static_cast<size_t>(px) * C + e % C]) >> shift);
        }
    }
    if (aligned && x0 + G::PX + 2 <= W) {
        unsigned w[(AP + 3) / 4];
        chroma_load<AP>(row + static_cast<size_t>(x0 + G::PX) * C, w);
#pragma unroll
        for (int e = 0; e < G::AE; ++e) v[G::AE + G::NE + e] = static_cast<float>(frame_elem<E>(w, e) >> shift);
    } else {
#pragma unroll
        for (int e = 0; e < G::AE; ++e) {
            const int px = min(x0 + G::PX + e / C, W - 1);
            v[G::AE + G::NE + e] = static_cast<float>(static_cast<unsigned>(row[static_cast<size_t>(px) * C + e % C]) >> shift);
        }
    }
}

// one staged row to the lane's R * PX output columns: output pixel j reads input pixel j / R at phase j % R, five weights over its offsets -2 .. 2
template <int R, int C, typename E>
__device__ __forceinline__ void chroma_hfilter(const ChromaParams& P, const float* v, float* h) {
    frame_hfilter<R, C, ChromaGeom<R, C, E>::PX>(P.wh, v, h);
}

template <int R, int C, typename E>
__device__ __forceinline__ void chroma_up_body(const ChromaParams& P, const E* __restrict__ in, E* __restrict__ out) {
    using G = ChromaGeom<R, C, E>;
    constexpr int ROWS = kChromaRows + 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = P.H, W = P.W, OH = R * P.H, OW = R * P.W;
    const FrameTile tile = frame_tile(blockIdx.x, P.tilesX, P.tilesY);
    const size_t n = tile.n;
    const int x0 = (tile.tx * 64 + lane) * G::PX;
    const int y0 = tile.ty * G::TILE_H + wave * kChromaRows;
    if (x0 >= W || y0 >= H) return; // (no barrier anywhere below)
    const E* plane = in + n * H * W * C;

    float h[ROWS][G::NV]; // input rows y0 - 2 .. y0 + kChromaRows + 1 (clamped), resampled to the lane's output columns
    constexpr int AP = G::AE * G::ES, APW = (AP + 3) / 4, INW = G::IN / 4;
    // an interior lane of a plane whose rows all start on a multiple of IN bytes: three aligned loads per row, all 3 * ROWS of them independent and
    // issued before the first is waited for (one branch for the lane, none per row)
    const bool rowsAligned = (reinterpret_cast<size_t>(plane) & (G::IN - 1)) == 0 && (static_cast<size_t>(W) * C * G::ES) % G::IN == 0;
    if (rowsAligned && x0 >= 2 && x0 + G::PX + 2 <= W) {
        unsigned raw[ROWS][INW + 2 * APW];
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int gy = min(max(y0 - 2 + i, 0), H - 1);
            const E* p = plane + static_cast<size_t>(gy) * W * C + static_cast<size_t>(x0) * C;
            chroma_load<AP>(p - G::AE, raw[i]);
            chroma_load<G::IN>(p, raw[i] + APW);
            chroma_load<AP>(p + G::NE, raw[i] + APW + INW);
        }
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            float v[G::NB];
#pragma unroll
            for (int e = 0; e < G::AE; ++e) {
                v[e] = static_cast<float>(frame_elem<E>(raw[i], e) >> P.shift);
                v[G::AE + G::NE + e] = static_cast<float>(frame_elem<E>(raw[i] + APW + INW, e) >> P.shift);
            }
#pragma unroll
            for (int e = 0; e < G::NE; ++e) v[G::AE + e] = static_cast<float>(frame_elem<E>(raw[i] + APW, e) >> P.shift);
            chroma_hfilter<R, C, E>(P, v, h[i]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int gy = min(max(y0 - 2 + i, 0), H - 1);
            float v[G::NB];
            chroma_load_row<R, C, E>(plane + static_cast<size_t>(gy) * W * C, x0, W, P.shift, v);
            chroma_hfilter<R, C, E>(P, v, h[i]);
        }
    }

    const bool full = x0 + G::PX <= W;
    const int valid = min(G::PX, W - x0) * R * C; // output elements of this lane inside the plane
#pragma unroll
    for (int t = 0; t < kChromaRows; ++t) {
        const int y = y0 + t;
        if (y >= H) break;
#pragma unroll
        for (int q = 0; q < R; ++q) {
            unsigned e[G::NV];
#pragma unroll
            for (int i = 0; i < G::NV; ++i) {
                float acc = P.wv[q][0] * h[t][i];
#pragma unroll
                for (int k = 1; k < 5; ++k) acc += P.wv[q][k] * h[t + k][i];
                e[i] = quantize_frame(acc, P.maxval) << P.shift;
            }
            E* orow = out + (n * OH + (static_cast<size_t>(R) * y + q)) * OW * C;
            E* dst = orow + static_cast<size_t>(R) * x0 * C;
            if (full && (reinterpret_cast<size_t>(orow) & 15) == 0) {
                constexpr int PER = 4 / G::ES;
                unsigned w[G::OUTB / 4];
#pragma unroll
                for (int k = 0; k < G::OUTB / 4; ++k) {
                    w[k] = 0u;
#pragma unroll
                    for (int j = 0; j < PER; ++j) w[k] |= e[k * PER + j] << (8 * G::ES * j);
                }
                if constexpr (G::OUTB == 16) {
                    *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
                } else if constexpr (G::OUTB == 32) {
                    reinterpret_cast<uint4*>(dst)[0] = make_uint4(w[0], w[1], w[2], w[3]);
                    reinterpret_cast<uint4*>(dst)[1] = make_uint4(w[4], w[5], w[6], w[7]);
                } else { // 24 bytes at a multiple of 24: 16 + 8 or 8 + 16, whichever puts the wide store on a 16-byte boundary
                    static_assert(G::OUTB == 24, "lane output is 16, 24 or 32 bytes");
                    if ((reinterpret_cast<size_t>(dst) & 15) == 0) {
                        *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
                        *reinterpret_cast<uint2*>(reinterpret_cast<unsigned char*>(dst) + 16) = make_uint2(w[4], w[5]);
                    } else {
                        *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
                        *reinterpret_cast<uint4*>(reinterpret_cast<unsigned char*>(dst) + 8) = make_uint4(w[2], w[3], w[4], w[5]);
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < G::NV; ++i)
                    if (i < valid) dst[i] = static_cast<E>(e[i]);
            }
        }
    }
}

template <int R, int C, typename E>
__global__ __launch_bounds__(256) void chroma_up_kernel(ChromaParams P, const E* __restrict__ in, E* __restrict__ out) {
    chroma_up_body<R, C, E>(P, in, out);
}

struct ChromaUpPlan : snnhip_plan {
    snnhip_chroma_up_desc d;
    ChromaParams P;

    template <typename E>
    void launch(const snnhip_tensor* in, snnhip_tensor* out) {
        const dim3 grid(static_cast<unsigned>(P.N) * static_cast<unsigned>(P.tilesX) * static_cast<unsigned>(P.tilesY));
        const E* src = reinterpret_cast<const E*>(in->data);
        E* dst = reinterpret_cast<E*>(out->data);
        dispatch_r_c<1, 2>(d.r, d.C, [&](auto R, auto C) {
            SNNHIP_LAUNCH((chroma_up_kernel<decltype(R)::value, decltype(C)::value, E>), grid, dim3(256), 0, ctx->stream, P, src, dst);
        });
    }

    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        SNNHIP_REQUIRE(nIn == 1, "chroma_up: expects 1 input, got %d", nIn);
        SNNHIP_REQUIRE(in[0]->dtype == d.dtype && out->dtype == d.dtype, "chroma_up: both tensors must have dtype %d, got %d and %d", d.dtype, in[0]->dtype, out->dtype);
        SNNHIP_REQUIRE(dims_match(in[0], d.N, d.H, d.W, d.C), "chroma_up: the input plane is %dx%dx%dx%d, the plan was built for %dx%dx%dx%d", in[0]->n, in[0]->h, in[0]->w,
                       in[0]->c, d.N, d.H, d.W, d.C);
        SNNHIP_REQUIRE(dims_match(out, d.N, d.r * d.H, d.r * d.W, d.C), "chroma_up: the output is %dx%dx%dx%d, expected %dx%dx%dx%d (r = %d times the input plane)", out->n,
                       out->h, out->w, out->c, d.N, d.r * d.H, d.r * d.W, d.C, d.r);
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

int snnhip_bicubic_taps_sited(int r, int siting, float* weights, int* base, int capacity) {
    // the output is itself a chroma grid of the same siting (bicubic_phase_sited): lead = off
    return fill_bicubic_taps("bicubic_taps_sited", r, r, siting, siting_offset(siting), siting_offset(siting), weights, base, capacity);
}

int snnhip_chroma_up_plan_create(snnhip_ctx* ctx, const snnhip_chroma_up_desc* desc, snnhip_plan** out) {
    SNNHIP_REQUIRE(ctx && desc && out, "chroma_up_plan_create: null argument");
    SNNHIP_REQUIRE(desc->N > 0 && desc->H > 0 && desc->W > 0, "chroma_up desc: bad dims %dx%dx%d", desc->N, desc->H, desc->W);
    SNNHIP_REQUIRE(desc->C == 1 || desc->C == 2, "chroma_up desc: %d channels (1: one plane of a planar format, 2: interleaved CbCr)", desc->C);
    SNNHIP_REQUIRE(desc->r >= 1 && desc->r <= 4, "chroma_up desc: r = %d (an integer 1..4)", desc->r);
    int bits = 0;
    const int fmt = check_sample_format("chroma_up desc", "planes", desc->dtype, desc->siting, desc->shift, desc->maxval, &bits);
    if (fmt != SNNHIP_OK) return fmt;
    int th = 0, tw = 0;
    chroma_tile(desc->r, desc->C, bits / 8, &th, &tw);
    const int tilesX = up_div(desc->W, tw), tilesY = up_div(desc->H, th);
    const double blocks = static_cast<double>(desc->N) * tilesX * tilesY;
    const double inElems = static_cast<double>(desc->N) * desc->H * desc->W * desc->C;
    const double outElems = inElems * desc->r * desc->r;
    SNNHIP_REQUIRE(blocks < 2147483648.0 && outElems < 9.0e15, "chroma_up desc: %dx%dx%d at r = %d is too large", desc->N, desc->H, desc->W, desc->r);
    float wh[16] = {0}, wv[16] = {0};
    int bh[4] = {0}, bv[4] = {0};
    int rc = snnhip_bicubic_taps_sited(desc->r, desc->siting, wh, bh, 16);
    if (rc == SNNHIP_OK) rc = snnhip_bicubic_taps_sited(desc->r, SNNHIP_SITING_CENTRE, wv, bv, 16);
    if (rc != SNNHIP_OK) return rc;
    auto* plan = new ChromaUpPlan();
    plan->ctx = ctx;
    plan->dtype = desc->dtype;
    plan->rawInput = desc->dtype;
    plan->rawOutput = desc->dtype;
    plan->d = *desc;
    plan->P = ChromaParams{};
    plan->P.N = desc->N;
    plan->P.H = desc->H;
    plan->P.W = desc->W;
    plan->P.tilesX = tilesX;
    plan->P.tilesY = tilesY;
    plan->P.shift = desc->shift;
    plan->P.maxval = static_cast<float>(desc->maxval);
    widen_taps(desc->r, wh, bh, plan->P.wh);
    widen_taps(desc->r, wv, bv, plan->P.wv);
    plan->inDims[0] = plan->outDims[0] = desc->N;
    plan->inDims[1] = desc->H;
    plan->inDims[2] = desc->W;
    plan->outDims[1] = desc->r * desc->H;
    plan->outDims[2] = desc->r * desc->W;
    plan->inDims[3] = plan->outDims[3] = desc->C;
    plan->bytes = (inElems + outElems) * (bits / 8); // the input once, the output once
    plan->flops = outElems * 2.0 * 4.0 * (1.0 + 1.0 / desc->r); // 4 taps per pass, the horizontal pass shared by r rows
    char buf[240];
    snprintf(buf, sizeof(buf), "chroma_up_u%d r=%d c=%d siting=%s tile=%dx%d %dx%d -> %dx%d maxval=%d shift=%d kernel=chroma_up_kernel", bits, desc->r, desc->C,
             desc->siting == SNNHIP_SITING_LEFT ? "left" : "centre", th, tw, desc->H, desc->W, desc->r * desc->H, desc->r * desc->W, desc->maxval, desc->shift);
    plan->desc = buf;
    *out = plan;
    return SNNHIP_OK;
}

} // extern "C"
