// frame_rgb_cbcr.hip -- the 4:2:0 chroma plane of an upscaled frame from the ORIGINAL low-resolution RGB frame: RGB8 / RGBA8 in, NV12 out around a
// luma-only model (include/snnhip.h: snnhip_rgb_cbcr_plan_create / snnhip_bicubic_taps_rgb420 / snnhip_rgb_cbcr_coefficients; DESIGN.md section
// 4.17).  The reference has no counterpart: its ESPCN demo converts on the CPU and writes a grey image, and the libyuv it vendors converts on the CPU.
//
//   rgb_cbcr:  U8 [N][H][W][C] (C = 3 or 4, alpha ignored) -> U8 [N][rH/2][rW/2][2] (Cb, Cr), r = 2..4.  Per low-resolution pixel dB = B - ylo,
//              dR = R - ylo with ylo = kr R + kg G + kb B unquantised (luma_f32, the function rgb_luma and ycc_merge call); both resampled to the
//              output chroma grid with the separable Keys cubic (a = -0.5, horizontal then vertical, replicate edge, horizontal axis sited);
//              Cb = 128 + cbs dB~, Cr = 128 + crs dR~, q = clamp(rint(.), 0, 255).
//
// The output grid has r / 2 samples per input pixel: the pattern of CbcrGeom<R> repeats every P outputs over S inputs, (P, S) = (1, 1), (3, 2), (2, 1).
// The kernel follows chroma_up_kernel: no LDS, no barrier.  One lane owns four input pixels of a row (4 * C bytes, one load of C dwords) and the 4, 6
// or 8 output chroma pixels over them (one store of 2, 3 or 4 dwords) in each output row of its wave; the two apron pixels either side are one more
// load of two dwords each, which covers them at either channel count (it hits the lines the neighbouring lanes load).  A wave is 64 lanes side by
// side: it turns S * T + 4 input rows into (dB, dR) pairs, filters them horizontally in registers -- an interior lane issues all its loads before it
// waits for the first -- and forms its P * T output rows from them.  The per-phase base (-1, 0 or 1) is folded into the tap table on the host: a
// phase is S + 4 weights over offsets -2 .. S + 1 from the period's first pixel, zeros where it does not read, so that every register index is a
// compile-time constant (a term 0 * v adds exactly nothing).  Rows whose address is not dword-aligned (the RGB8 pitch 3W for W not a multiple of 4;
// the output pitch 2 * rW / 2 for odd rW / 2), the lane that straddles the right edge and aprons outside the frame take a byte path with clamped
// indices.
//
//   rgb_cbcr_planar (snnhip_rgb_cbcr_planar_plan_create): the same into two planes U8 [2N][rH/2][rW/2][1] (I420).  Only the
//              store side differs: the PLANAR branch of rgb_cbcr_body.
#include "frame_rgb_cbcr.h"
#include "plan_util.h"
#include "snnhip_internal.h"

namespace snnhip {
namespace {

struct RgbCbcrParams {
    int N, H, W;    // the LOW-resolution RGB frame
    int OH, OW;     // the output chroma plane: rH / 2, rW / 2
    int tilesX, tilesY;
    float kr, kg, kb;
    RgbCbcrCoeffs m;
    float wh[3][6]; // [phase][offset -2 .. 3] along a row (the desc's siting); rows P.. and columns S + 4.. unused
    float wv[3][6]; // ... along a column (centred)
};

// v[e * 2] = dB, v[e * 2 + 1] = dR of staged pixel e, from its three bytes
__device__ __forceinline__ void cbcr_differences(const RgbCbcrParams& P, unsigned r, unsigned g, unsigned b, float* v) {
    const float fr = static_cast<float>(r), fg = static_cast<float>(g), fb = static_cast<float>(b);
    const float yl = luma_f32(fr, fg, fb, P.kr, P.kg, P.kb);
    v[0] = fb - yl;
    v[1] = fr - yl;
}

// One staged row (NB pixels of (dB, dR): two pixels of apron either side) to the lane's OPX output pixels: output pixel j is phase j % P of period
// j / P, TAPS weights over the pixels from S * (j / P) on
template <int R>
__device__ __forceinline__ void cbcr_hfilter(const RgbCbcrParams& P, const float* v, float* h) {
    using G = CbcrGeom<R>;
#pragma unroll
    for (int j = 0; j < G::OPX; ++j) {
        const int x = G::S * (j / G::P), p = j % G::P;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float acc = P.wh[p][0] * v[x * 2 + c];
#pragma unroll
            for (int k = 1; k < G::TAPS; ++k) acc += P.wh[p][k] * v[(x + k) * 2 + c];
            h[j * 2 + c] = acc;
        }
    }
}

// PLANAR (snnhip_rgb_cbcr_planar_plan_create): the output is U8 [2N][OH][OW][1], plane 2n = Cb, 2n + 1 = Cr of image n.  The load and filter side is
// the interleaved kernel's; the lane's OPX Cb bytes and OPX Cr bytes go to the two planes, OPX bytes into each row from OPX * (its index in the row):
// whole dwords where that row of that plane starts on one (OPX = 4, 8 at r = 2, 4), halfwords at r = 3 (OPX = 6) on an even address, bytes otherwise
template <int R, int C, bool PLANAR = false>
__device__ __forceinline__ void rgb_cbcr_body(const RgbCbcrParams& P, const unsigned char* __restrict__ in, unsigned char* __restrict__ out) {
    using G = CbcrGeom<R>;
    constexpr int NW = C + 4;       // dwords that cover the lane's staged pixels of a row: 8 bytes, the lane's own 4 * C, 8 bytes
    constexpr int OFF = 8 - 2 * C;  // byte of staged pixel 0 (x0 - 2) in them
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = P.H, W = P.W;
    const FrameTile tile = frame_tile(blockIdx.x, P.tilesX, P.tilesY);
    const size_t n = tile.n;
    const int x0 = (tile.tx * 64 + lane) * kCbcrIn;                  // first input pixel of the lane
    const int py0 = (tile.ty * kCbcrWaves + wave) * G::T;            // first vertical period of the wave
    const int y0 = G::S * py0;                                       // ... its first input row
    if (x0 >= W || y0 >= H) return; // (no barrier anywhere below)
    const unsigned char* plane = in + n * H * W * C;

    float h[G::ROWS][G::OPX * 2]; // input rows y0 - 2 .. y0 + S * T + 1 (clamped) as (dB, dR), resampled to the lane's output columns
    // an interior lane of a frame whose rows all start on a dword: three loads per row, all 3 * ROWS of them independent and issued before the first is
    // waited for.  The last of them ends 4 * C + 8 bytes past the lane's first byte: inside the row for x0 + 7 <= W at either channel count
    const bool rowsAligned = (reinterpret_cast<size_t>(plane) & 3) == 0 && (static_cast<size_t>(W) * C) % 4 == 0;
    if (rowsAligned && x0 >= 4 && x0 + kCbcrIn + 3 <= W) {
        unsigned raw[G::ROWS][NW];
#pragma unroll
        for (int i = 0; i < G::ROWS; ++i) {
            const int gy = min(max(y0 - 2 + i, 0), H - 1);
            const unsigned char* p = plane + (static_cast<size_t>(gy) * W + x0) * C;
            load_words<2>(p - 8, raw[i]);
            load_words<C>(p, raw[i] + 2);
            load_words<2>(p + kCbcrIn * C, raw[i] + 2 + C);
        }
#pragma unroll
        for (int i = 0; i < G::ROWS; ++i) {
            float v[G::NB * 2];
#pragma unroll
            for (int e = 0; e < G::NB; ++e) {
                const int b = OFF + e * C;
                cbcr_differences(P, frame_elem<unsigned char>(raw[i], b), frame_elem<unsigned char>(raw[i], b + 1), frame_elem<unsigned char>(raw[i], b + 2), v + e * 2);
            }
            cbcr_hfilter<R>(P, v, h[i]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < G::ROWS; ++i) {
            const int gy = min(max(y0 - 2 + i, 0), H - 1);
            const unsigned char* row = plane + static_cast<size_t>(gy) * W * C;
            float v[G::NB * 2];
#pragma unroll
            for (int e = 0; e < G::NB; ++e) {
                const unsigned char* p = row + static_cast<size_t>(min(max(x0 - 2 + e, 0), W - 1)) * C;
                cbcr_differences(P, p[0], p[1], p[2], v + e * 2);
            }
            cbcr_hfilter<R>(P, v, h[i]);
        }
    }

    const int periods = min(G::K, (W - x0) / G::S); // whole periods of this lane inside the frame (W is a multiple of S)
    const bool full = periods == G::K;
    const int valid = periods * G::P * 2;           // output bytes of this lane inside the plane
    const size_t col0 = static_cast<size_t>(G::OPX) * (static_cast<size_t>(tile.tx) * 64 + lane);
#pragma unroll
    for (int t = 0; t < G::T; ++t) {
        if (G::S * (py0 + t) >= H) break;
#pragma unroll
        for (int q = 0; q < G::P; ++q) {
            unsigned e[G::OPX * 2];
#pragma unroll
            for (int i = 0; i < G::OPX * 2; ++i) {
                float acc = P.wv[q][0] * h[G::S * t][i];
#pragma unroll
                for (int k = 1; k < G::TAPS; ++k) acc += P.wv[q][k] * h[G::S * t + k][i];
                e[i] = quantize_frame(P.m.coff + (i % 2 ? P.m.crs : P.m.cbs) * acc, 255.0f);
            }
            const size_t J = static_cast<size_t>(G::P) * (py0 + t) + q;
            if constexpr (PLANAR) {
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    unsigned char* prow = out + ((2 * n + c) * P.OH + J) * P.OW; // (the Cr plane lies OH * OW bytes behind Cb: its rows align on their own)
                    unsigned char* dst = prow + col0;
                    const size_t al = reinterpret_cast<size_t>(prow);
                    if (full && G::OPX % 4 == 0 && (al & 3) == 0) {
                        unsigned w[(G::OPX + 3) / 4];
#pragma unroll
                        for (int k = 0; k < G::OPX / 4; ++k) w[k] = e[8 * k + c] | (e[8 * k + 2 + c] << 8) | (e[8 * k + 4 + c] << 16) | (e[8 * k + 6 + c] << 24);
                        store_words<(G::OPX + 3) / 4>(dst, w);
                    } else if (full && (al & 1) == 0) { // (OPX is even: the piece starts on a halfword)
#pragma unroll
                        for (int k = 0; k < G::OPX / 2; ++k) reinterpret_cast<unsigned short*>(dst)[k] = static_cast<unsigned short>(e[4 * k + c] | (e[4 * k + 2 + c] << 8));
                    } else {
#pragma unroll
                        for (int i = 0; i < G::OPX; ++i)
                            if (i * 2 < valid) dst[i] = static_cast<unsigned char>(e[i * 2 + c]);
                    }
                }
                continue;
            }
            unsigned char* orow = out + (n * P.OH + J) * P.OW * 2;
            unsigned char* dst = orow + col0 * 2;
            if (full && (reinterpret_cast<size_t>(orow) & 3) == 0) { // the lane's piece starts a multiple of 4 bytes into the row
                unsigned w[G::OW];
#pragma unroll
                for (int k = 0; k < G::OW; ++k) w[k] = e[4 * k] | (e[4 * k + 1] << 8) | (e[4 * k + 2] << 16) | (e[4 * k + 3] << 24);
                store_words<G::OW>(dst, w);
            } else {
#pragma unroll
                for (int i = 0; i < G::OPX * 2; ++i)
                    if (i < valid) dst[i] = static_cast<unsigned char>(e[i]);
            }
        }
    }
}

template <int R, int C>
__global__ __launch_bounds__(256) void rgb_cbcr_kernel(RgbCbcrParams P, const unsigned char* __restrict__ in, unsigned char* __restrict__ out) {
    if constexpr (R >= 2) rgb_cbcr_body<R, C>(P, in, out); // (dispatch_r_c names r = 1 too; the plan refuses it)
}

template <int R, int C>
__global__ __launch_bounds__(256) void rgb_cbcr_planar_kernel(RgbCbcrParams P, const unsigned char* __restrict__ in, unsigned char* __restrict__ out) {
    if constexpr (R >= 2) rgb_cbcr_body<R, C, true>(P, in, out);
}

struct RgbCbcrPlan : snnhip_plan {
    snnhip_rgb_cbcr_desc d;
    RgbCbcrParams P;
    bool planar = false; // the output is [2N][OH][OW][1] (snnhip_rgb_cbcr_planar_plan_create)

    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        if (planar) {
            SNNHIP_REQUIRE(nIn == 1, "rgb_cbcr_planar: expects 1 input, got %d", nIn);
            SNNHIP_REQUIRE(in[0]->dtype == SNNHIP_U8 && out->dtype == SNNHIP_U8, "rgb_cbcr_planar: both tensors must be SNNHIP_U8, got dtypes %d and %d", in[0]->dtype, out->dtype);
            SNNHIP_REQUIRE(dims_match(in[0], d.N, d.H, d.W, d.C), "rgb_cbcr_planar: the input frame is %dx%dx%dx%d, the plan was built for %dx%dx%dx%d", in[0]->n, in[0]->h,
                           in[0]->w, in[0]->c, d.N, d.H, d.W, d.C);
            SNNHIP_REQUIRE(dims_match(out, 2 * d.N, P.OH, P.OW, 1),
                           "rgb_cbcr_planar: the output is %dx%dx%dx%d, expected %dx%dx%dx1 ([2N][rH/2][rW/2][1]: the Cb and Cr planes of a %dx%d frame, r = %d)", out->n, out->h,
                           out->w, out->c, 2 * d.N, P.OH, P.OW, d.r * d.H, d.r * d.W, d.r);
        } else {
            SNNHIP_REQUIRE(nIn == 1, "rgb_cbcr: expects 1 input, got %d", nIn);
            SNNHIP_REQUIRE(in[0]->dtype == SNNHIP_U8 && out->dtype == SNNHIP_U8, "rgb_cbcr: both tensors must be SNNHIP_U8, got dtypes %d and %d", in[0]->dtype, out->dtype);
            SNNHIP_REQUIRE(dims_match(in[0], d.N, d.H, d.W, d.C), "rgb_cbcr: the input frame is %dx%dx%dx%d, the plan was built for %dx%dx%dx%d", in[0]->n, in[0]->h, in[0]->w,
                           in[0]->c, d.N, d.H, d.W, d.C);
            SNNHIP_REQUIRE(dims_match(out, d.N, P.OH, P.OW, 2), "rgb_cbcr: the output is %dx%dx%dx%d, expected %dx%dx%dx2 (the chroma plane of a %dx%d frame, r = %d)", out->n, out->h,
                           out->w, out->c, d.N, P.OH, P.OW, d.r * d.H, d.r * d.W, d.r);
        }
        const dim3 grid(static_cast<unsigned>(P.N) * static_cast<unsigned>(P.tilesX) * static_cast<unsigned>(P.tilesY));
        const unsigned char* src = reinterpret_cast<const unsigned char*>(in[0]->data);
        unsigned char* dst = reinterpret_cast<unsigned char*>(out->data);
        dispatch_r_c<3, 4>(d.r, d.C, [&](auto R, auto C) {
            if (planar) SNNHIP_LAUNCH((rgb_cbcr_planar_kernel<decltype(R)::value, decltype(C)::value>), grid, dim3(256), 0, ctx->stream, P, src, dst);
            else SNNHIP_LAUNCH((rgb_cbcr_kernel<decltype(R)::value, decltype(C)::value>), grid, dim3(256), 0, ctx->stream, P, src, dst);
        });
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }
};

// a phase's four weights at base - 1 .. base + 2 as six weights over -2 .. 3 (w6 zeroed by the caller), as widen_taps does for bases -1 and 0
void widen_taps6(int phases, const float* w4, const int* base, float (&w6)[3][6]) {
    for (int p = 0; p < phases; ++p)
        for (int k = 0; k < 4; ++k) w6[p][base[p] + 1 + k] = w4[4 * p + k];
}

} // namespace
} // namespace snnhip

using namespace snnhip;

extern "C" {

int snnhip_bicubic_taps_rgb420(int r, int siting, float* weights, int* base, int capacity) {
    SNNHIP_REQUIRE(r >= 2 && r <= 4, "bicubic_taps_rgb420: r = %d (2..4: at r = 1 the chroma grid is half the frame's, which needs a decimation filter)", r);
    // output P x' + p reads S x' + s_p, s_p = (2p + lead) / r - 0.5: two luma columns per output, lead by the siting
    return fill_bicubic_taps("bicubic_taps_rgb420", r, rgb420_phases(r), siting, rgb420_lead(siting), 0.5, weights, base, capacity, 2, r, 1);
}

int snnhip_rgb_cbcr_coefficients(int range, float kr, float kb, float* out, int capacity) {
    SNNHIP_REQUIRE(out, "rgb_cbcr_coefficients: null argument");
    SNNHIP_REQUIRE(capacity >= 3, "rgb_cbcr_coefficients: room for %d floats, 3 needed", capacity);
    SNNHIP_REQUIRE(range == SNNHIP_RANGE_LIMITED || range == SNNHIP_RANGE_FULL, "rgb_cbcr_coefficients: range %d (SNNHIP_RANGE_LIMITED or SNNHIP_RANGE_FULL)", range);
    SNNHIP_REQUIRE(matrix_ok(kr, kb), "rgb_cbcr_coefficients: kr = %g, kb = %g (0 < kr, 0 < kb, kr + kb < 1)", kr, kb);
    const RgbCbcrCoeffs c = rgb_cbcr_coeffs(range, kr, kb);
    out[0] = c.coff, out[1] = c.cbs, out[2] = c.crs;
    return SNNHIP_OK;
}

// snnhip_rgb_cbcr_plan_create and snnhip_rgb_cbcr_planar_plan_create: one desc, one set of checks, tables and coefficients (the messages speak of
// "rgb_cbcr desc" for both: it is the same struct)
static int rgb_cbcr_plan_make(snnhip_ctx* ctx, const snnhip_rgb_cbcr_desc* desc, snnhip_plan** out, bool planar) {
    SNNHIP_REQUIRE(ctx && desc && out, "%s: null argument", planar ? "rgb_cbcr_planar_plan_create" : "rgb_cbcr_plan_create");
    SNNHIP_REQUIRE(desc->N > 0 && desc->H > 0 && desc->W > 0, "rgb_cbcr desc: bad dims %dx%dx%d", desc->N, desc->H, desc->W);
    SNNHIP_REQUIRE(desc->C == 3 || desc->C == 4, "rgb_cbcr desc: %d channels (3: RGB8, 4: RGBA8)", desc->C);
    SNNHIP_REQUIRE(desc->r != 1, "rgb_cbcr desc: r = 1 would halve the chroma grid, which needs a decimation filter: not built (r is 2..4)");
    SNNHIP_REQUIRE(desc->r >= 2 && desc->r <= 4, "rgb_cbcr desc: r = %d (an integer 2..4)", desc->r);
    SNNHIP_REQUIRE(siting_ok(desc->siting), "rgb_cbcr desc: siting %d (SNNHIP_SITING_CENTRE or SNNHIP_SITING_LEFT)", desc->siting);
    SNNHIP_REQUIRE(desc->range == SNNHIP_RANGE_LIMITED || desc->range == SNNHIP_RANGE_FULL, "rgb_cbcr desc: range %d (SNNHIP_RANGE_LIMITED or SNNHIP_RANGE_FULL)", desc->range);
    SNNHIP_REQUIRE(matrix_ok(desc->kr, desc->kb), "rgb_cbcr desc: kr = %g, kb = %g (0 < kr, 0 < kb, kr + kb < 1)", desc->kr, desc->kb);
    const double oh2 = static_cast<double>(desc->r) * desc->H, ow2 = static_cast<double>(desc->r) * desc->W;
    SNNHIP_REQUIRE(oh2 < 2147483648.0 && ow2 < 2147483648.0, "rgb_cbcr desc: %dx%dx%d at r = %d is too large", desc->N, desc->H, desc->W, desc->r);
    SNNHIP_REQUIRE((desc->r * desc->H) % 2 == 0 && (desc->r * desc->W) % 2 == 0, "rgb_cbcr desc: the output frame %dx%d (r = %d) has an odd extent: no 4:2:0 chroma plane", desc->r * desc->H,
                   desc->r * desc->W, desc->r);
    const int OH = desc->r * desc->H / 2, OW = desc->r * desc->W / 2;
    int th = 0, tw = 0;
    rgb_cbcr_tile(desc->r, &th, &tw);
    const int tilesX = up_div(OW, tw), tilesY = up_div(OH, th);
    const double blocks = static_cast<double>(desc->N) * tilesX * tilesY;
    const double inBytes = static_cast<double>(desc->N) * desc->H * desc->W * desc->C;
    const double outBytes = static_cast<double>(desc->N) * OH * OW * 2.0;
    SNNHIP_REQUIRE(blocks < 2147483648.0 && inBytes < 9.0e15 && outBytes < 9.0e15, "rgb_cbcr desc: %dx%dx%d at r = %d is too large", desc->N, desc->H, desc->W, desc->r);
    float wh[12] = {0}, wv[12] = {0};
    int bh[3] = {0}, bv[3] = {0};
    int rc = snnhip_bicubic_taps_rgb420(desc->r, desc->siting, wh, bh, 12);
    if (rc == SNNHIP_OK) rc = snnhip_bicubic_taps_rgb420(desc->r, SNNHIP_SITING_CENTRE, wv, bv, 12);
    if (rc != SNNHIP_OK) return rc;
    auto* plan = new RgbCbcrPlan();
    plan->ctx = ctx;
    plan->dtype = SNNHIP_U8;
    plan->rawInput = SNNHIP_U8;
    plan->rawOutput = SNNHIP_U8;
    plan->d = *desc;
    plan->planar = planar;
    plan->P = RgbCbcrParams{};
    plan->P.N = desc->N;
    plan->P.H = desc->H;
    plan->P.W = desc->W;
    plan->P.OH = OH;
    plan->P.OW = OW;
    plan->P.tilesX = tilesX;
    plan->P.tilesY = tilesY;
    plan->P.kr = desc->kr;
    plan->P.kg = static_cast<float>(1.0 - static_cast<double>(desc->kr) - static_cast<double>(desc->kb)); // (as rgb_luma and ycc_merge form it)
    plan->P.kb = desc->kb;
    plan->P.m = rgb_cbcr_coeffs(desc->range, desc->kr, desc->kb);
    widen_taps6(rgb420_phases(desc->r), wh, bh, plan->P.wh);
    widen_taps6(rgb420_phases(desc->r), wv, bv, plan->P.wv);
    plan->inDims[0] = plan->outDims[0] = desc->N;
    plan->inDims[1] = desc->H;
    plan->inDims[2] = desc->W;
    plan->inDims[3] = desc->C;
    plan->outDims[1] = OH;
    plan->outDims[2] = OW;
    plan->outDims[3] = 2;
    if (planar) plan->outDims[0] = 2 * desc->N, plan->outDims[3] = 1;
    plan->bytes = inBytes + outBytes; // the input once, the output once
    const double inPixels = static_cast<double>(desc->N) * desc->H * desc->W;
    plan->flops = inPixels * 7.0 + outBytes * (2.0 * 4.0 * (1.0 + 2.0 / desc->r) + 2.0); // the differences; 4 taps per pass (the horizontal pass on 2 / r rows per output row); the scale
    char buf[280];
    snprintf(buf, sizeof(buf), "%s r=%d c=%d siting=%s range=%s tile=%dx%d %dx%d -> %dx%d kr=%g kb=%g kernel=%s", planar ? "rgb_cbcr_planar_u8" : "rgb_cbcr_u8", desc->r, desc->C,
             desc->siting == SNNHIP_SITING_LEFT ? "left" : "centre", desc->range == SNNHIP_RANGE_LIMITED ? "limited" : "full", th, tw, desc->H, desc->W, OH, OW, desc->kr, desc->kb, planar ? "rgb_cbcr_planar_kernel" : "rgb_cbcr_kernel");
    plan->desc = buf;
    *out = plan;
    return SNNHIP_OK;
}

int snnhip_rgb_cbcr_plan_create(snnhip_ctx* ctx, const snnhip_rgb_cbcr_desc* desc, snnhip_plan** out) { return rgb_cbcr_plan_make(ctx, desc, out, false); }

int snnhip_rgb_cbcr_planar_plan_create(snnhip_ctx* ctx, const snnhip_rgb_cbcr_desc* desc, snnhip_plan** out) { return rgb_cbcr_plan_make(ctx, desc, out, true); }

} // extern "C"
