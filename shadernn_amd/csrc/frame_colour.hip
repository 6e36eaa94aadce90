// frame_colour.hip -- colour frames around a luma-only model (include/snnhip.h: snnhip_rgb_luma_plan_create / snnhip_ycc_merge_plan_create /
// snnhip_bicubic_taps).  The reference's ESPCN demo converts BGR -> YCrCb on the CPU, feeds Y and writes a grey image
// (demo/modelInferenceESPCN.py); here the two maps either side of the model are device kernels on interleaved 8-bit frames:
//
//   rgb_luma :  U8 [P][C] -> U8 [P][1],  q = clamp(rint(kr*R + kg*G + kb*B), 0, 255)                      (P = N*H*W pixels, C = 3 or 4)
//   ycc_merge:  Yhi U8 [N][rH][rW][1] + the low-resolution frame U8 [N][H][W][C] -> U8 [N][rH][rW][C]
//               (dR, dB) = (R - ylo, B - ylo) per low-resolution pixel, resampled with the separable Catmull-Rom filter (aligned pixel centres, replicate
//               edge), R' = Yhi + dR~, B' = Yhi + dB~, G' = Yhi - (kr*dR~ + kb*dB~) / kg, each quantised; alpha copied from the pixel underneath.
//
// Both are HBM-bound.  The luma map is a grid-stride stream: one lane takes 4 pixels = C dwords in, one dword out; pixels that do not fill a group (and
// everything when a base pointer is not dword-aligned) take a byte path.  The merge kernel works on low-resolution tiles of kMergeTileH x
// kMergeTileW pixels, one 256-thread block each:
//   1. stage (TH + 4) x (TW + 4) pairs (dR, dB) in LDS, coordinates clamped to the frame (an output sample r*x + p reads low-resolution x - 2 .. x + 1 or
//      x - 1 .. x + 2 depending on its phase p: two pixels of apron on every side);
//   2. horizontal pass: every staged row to r*TW output columns, into a second LDS array (one thread per low-resolution pixel: its five neighbours
//      once, r phases with the tap weights as uniform constants);
//   3. vertical pass: one thread per low-resolution row and group of 4 output columns reads five rows of the second array and produces the r output
//      rows of the group: a dword of Yhi in, 4 pixels = C dwords out per row.  A row whose address is not dword-aligned (the RGB8 pitch 3*r*W is odd for
//      odd r*W) and the ragged right edge take byte loads and stores.
// Element type E is a template parameter (16-bit colour frames are a later step); only unsigned char is instantiated.
#include "frame_colour.h"
#include "plan_util.h"
#include "snnhip_internal.h"

namespace snnhip {
namespace {

// i0 of phase p relative to the low-resolution pixel underneath, floor((p + 0.5) / r - 0.5): -1 or 0 (bicubic_phase computes the same on the host)
constexpr int phase_first(int r, int p) { return 2 * p + 1 < r ? -1 : 0; }

// (a kernel parameter: the type stays in this unit's unnamed namespace, where the kernels' symbols have it)
struct ColourMatrix {
    float kr, kg, kb;
};

struct MergeParams {
    int N, H, W; // the LOW-resolution frame
    int tilesX, tilesY;
    ColourMatrix m;
    float w[4][4]; // [phase][tap], rows r.. unused
};

template <int C, typename E>
__device__ __forceinline__ void rgb_luma_body(size_t pixels, ColourMatrix m, const E* __restrict__ x, E* __restrict__ y) {
    const float maxval = FrameElem<E>::maxval;
    const bool wide = sizeof(E) == 1 && ((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(y)) & 3) == 0;
    const size_t groups = wide ? pixels / 4 : 0;
    const size_t stride = static_cast<size_t>(gridDim.x) * 256;
    const size_t first = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    for (size_t g = first; g < groups; g += stride) {
        unsigned w[C];
#pragma unroll
        for (int k = 0; k < C; ++k) w[k] = reinterpret_cast<const unsigned*>(x)[g * C + k];
        unsigned q = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int e = j * C + c;
                v[c] = static_cast<float>((w[e >> 2] >> (8 * (e & 3))) & 255u);
            }
            q |= quantize_frame(luma_f32(v[0], v[1], v[2], m.kr, m.kg, m.kb), maxval) << (8 * j);
        }
        reinterpret_cast<unsigned*>(y)[g] = q;
    }
    for (size_t i = groups * 4 + first; i < pixels; i += stride) {
        const E* p = x + i * C;
        y[i] = static_cast<E>(quantize_frame(luma_f32(static_cast<float>(p[0]), static_cast<float>(p[1]), static_cast<float>(p[2]), m.kr, m.kg, m.kb), maxval));
    }
}

template <int C>
__global__ __launch_bounds__(256) void rgb_luma_u8_kernel(size_t pixels, ColourMatrix m, const unsigned char* __restrict__ x, unsigned char* __restrict__ y) {
    rgb_luma_body<C, unsigned char>(pixels, m, x, y);
}

template <int R, int C, typename E>
__device__ __forceinline__ void ycc_merge_body(const MergeParams& P, const E* __restrict__ yhi, const E* __restrict__ lo, E* __restrict__ out) {
    constexpr int TH = kMergeTileH, TW = kMergeTileW, SH = TH + 4, SW = TW + 4, OT = R * TW, GROUPS = OT / 4;
    __shared__ float2 s0[SH][SW];  // (dR, dB) of low-resolution pixels (y0 - 2 + ly, x0 - 2 + lx), clamped
    __shared__ float2 hp[SH][OT];  // the same rows, resampled to the tile's output columns
    __shared__ E alpha[C == 4 ? TH : 1][C == 4 ? TW : 1];
    const float maxval = FrameElem<E>::maxval;
    const int tid = threadIdx.x;
    const int H = P.H, W = P.W, OH = R * P.H, OW = R * P.W;
    const FrameTile tile = frame_tile(blockIdx.x, P.tilesX, P.tilesY);
    const size_t n = tile.n;
    const int x0 = tile.tx * TW, y0 = tile.ty * TH;
    const bool loWide = C == 4 && sizeof(E) == 1 && (reinterpret_cast<size_t>(lo) & 3) == 0;

    for (int i = tid; i < SH * SW; i += 256) {
        const int ly = i / SW, lx = i - ly * SW;
        const int gy = min(max(y0 - 2 + ly, 0), H - 1), gx = min(max(x0 - 2 + lx, 0), W - 1);
        const E* p = lo + ((n * H + gy) * W + gx) * C;
        float r, g, bl;
        unsigned a = 0u;
        if (loWide) {
            const unsigned v = *reinterpret_cast<const unsigned*>(p);
            r = static_cast<float>(v & 255u);
            g = static_cast<float>((v >> 8) & 255u);
            bl = static_cast<float>((v >> 16) & 255u);
            a = v >> 24;
        } else {
            r = static_cast<float>(p[0]);
            g = static_cast<float>(p[1]);
            bl = static_cast<float>(p[2]);
            if (C == 4) a = p[3];
        }
        const float yl = luma_f32(r, g, bl, P.m.kr, P.m.kg, P.m.kb);
        s0[ly][lx] = make_float2(r - yl, bl - yl);
        if (C == 4 && ly >= 2 && ly < 2 + TH && lx >= 2 && lx < 2 + TW) alpha[ly - 2][lx - 2] = static_cast<E>(a);
    }
    __syncthreads();

    for (int i = tid; i < SH * TW; i += 256) {
        const int ly = i / TW, x = i - ly * TW;
        float2 v[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] = s0[ly][x + k]; // low-resolution x0 + x - 2 .. x0 + x + 2
#pragma unroll
        for (int p = 0; p < R; ++p) {
            const int f = phase_first(R, p) + 1; // taps v[f] .. v[f + 3]
            float2 acc;
            acc.x = P.w[p][0] * v[f].x + P.w[p][1] * v[f + 1].x + P.w[p][2] * v[f + 2].x + P.w[p][3] * v[f + 3].x;
            acc.y = P.w[p][0] * v[f].y + P.w[p][1] * v[f + 1].y + P.w[p][2] * v[f + 2].y + P.w[p][3] * v[f + 3].y;
            hp[ly][R * x + p] = acc;
        }
    }
    __syncthreads();

    for (int i = tid; i < TH * GROUPS; i += 256) {
        const int y = i / GROUPS, xl = 4 * (i - y * GROUPS);
        const int gy = y0 + y, X = R * x0 + xl;
        if (gy >= H || X >= OW) continue;
        const int valid = min(4, OW - X);
        float2 v[5][4];
#pragma unroll
        for (int k = 0; k < 5; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[k][j] = hp[y + k][xl + j]; // low-resolution rows y0 + y - 2 .. y0 + y + 2
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int f = phase_first(R, q) + 1;
            const size_t pix = (n * OH + (static_cast<size_t>(R) * gy + q)) * OW + X;
            const E* ysrc = yhi + pix;
            E* dst = out + pix * C;
            float yh[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (sizeof(E) == 1 && valid == 4 && (reinterpret_cast<size_t>(ysrc) & 3) == 0) {
                const unsigned u = *reinterpret_cast<const unsigned*>(ysrc);
#pragma unroll
                for (int j = 0; j < 4; ++j) yh[j] = static_cast<float>((u >> (8 * j)) & 255u);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < valid) yh[j] = static_cast<float>(ysrc[j]);
            }
            unsigned e[4][C];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float dr = P.w[q][0] * v[f][j].x + P.w[q][1] * v[f + 1][j].x + P.w[q][2] * v[f + 2][j].x + P.w[q][3] * v[f + 3][j].x;
                const float db = P.w[q][0] * v[f][j].y + P.w[q][1] * v[f + 1][j].y + P.w[q][2] * v[f + 2][j].y + P.w[q][3] * v[f + 3][j].y;
                e[j][0] = quantize_frame(yh[j] + dr, maxval);
                e[j][1] = quantize_frame(yh[j] - (P.m.kr * dr + P.m.kb * db) / P.m.kg, maxval);
                e[j][2] = quantize_frame(yh[j] + db, maxval);
                if (C == 4) e[j][3] = alpha[y][(xl + j) / R];
            }
            if (sizeof(E) == 1 && valid == 4 && (reinterpret_cast<size_t>(dst) & 3) == 0) {
                unsigned w[C];
#pragma unroll
                for (int k = 0; k < C; ++k) w[k] = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const int by = j * C + c;
                        w[by >> 2] |= e[j][c] << (8 * (by & 3));
                    }
                if (C == 4 && (reinterpret_cast<size_t>(dst) & 15) == 0) {
                    *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3 % C]);
                } else {
#pragma unroll
                    for (int k = 0; k < C; ++k) reinterpret_cast<unsigned*>(dst)[k] = w[k];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < valid) {
#pragma unroll
                        for (int c = 0; c < C; ++c) dst[j * C + c] = static_cast<E>(e[j][c]);
                    }
            }
        }
    }
}

template <int R, int C>
__global__ __launch_bounds__(256) void ycc_merge_u8_kernel(MergeParams P, const unsigned char* __restrict__ yhi, const unsigned char* __restrict__ lo,
                                                           unsigned char* __restrict__ out) {
    ycc_merge_body<R, C, unsigned char>(P, yhi, lo, out);
}

ColourMatrix make_matrix(float kr, float kb) {
    return ColourMatrix{kr, static_cast<float>(1.0 - static_cast<double>(kr) - static_cast<double>(kb)), kb};
}

const unsigned char* bytes_of(const snnhip_tensor* t) { return reinterpret_cast<const unsigned char*>(t->data); }

struct RgbLumaPlan : snnhip_plan {
    snnhip_rgb_luma_desc d;
    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        SNNHIP_REQUIRE(nIn == 1, "rgb_luma: expects 1 input, got %d", nIn);
        SNNHIP_REQUIRE(in[0]->dtype == SNNHIP_U8 && out->dtype == SNNHIP_U8, "rgb_luma: both tensors must be SNNHIP_U8, got dtypes %d and %d", in[0]->dtype, out->dtype);
        SNNHIP_REQUIRE(dims_match(in[0], d.N, d.H, d.W, d.C) && dims_match(out, d.N, d.H, d.W, 1), "rgb_luma: tensor dims do not match the plan");
        const size_t pixels = static_cast<size_t>(d.N) * d.H * d.W;
        const ColourMatrix m = make_matrix(d.kr, d.kb);
        const unsigned g = grid_for(ctx, pixels / 4 + 1);
        unsigned char* dst = reinterpret_cast<unsigned char*>(out->data);
        if (d.C == 3) SNNHIP_LAUNCH((rgb_luma_u8_kernel<3>), dim3(g), dim3(256), 0, ctx->stream, pixels, m, bytes_of(in[0]), dst);
        else SNNHIP_LAUNCH((rgb_luma_u8_kernel<4>), dim3(g), dim3(256), 0, ctx->stream, pixels, m, bytes_of(in[0]), dst);
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }
};

struct YccMergePlan : snnhip_plan {
    snnhip_ycc_merge_desc d;
    MergeParams P;
    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        SNNHIP_REQUIRE(nIn == 2, "ycc_merge: expects 2 inputs (Yhi, the low-resolution frame), got %d", nIn);
        SNNHIP_REQUIRE(in[0]->dtype == SNNHIP_U8 && in[1]->dtype == SNNHIP_U8 && out->dtype == SNNHIP_U8, "ycc_merge: every tensor must be SNNHIP_U8, got dtypes %d, %d and %d",
                       in[0]->dtype, in[1]->dtype, out->dtype);
        SNNHIP_REQUIRE(dims_match(in[1], d.N, d.H, d.W, d.C), "ycc_merge: the low-resolution frame is %dx%dx%dx%d, the plan was built for %dx%dx%dx%d", in[1]->n, in[1]->h,
                       in[1]->w, in[1]->c, d.N, d.H, d.W, d.C);
        // r follows from the two shapes: an integer 1..4, the same on both axes -- and the one the plan was built for
        SNNHIP_REQUIRE(in[0]->n == d.N && in[0]->c == 1 && in[0]->h == d.r * d.H && in[0]->w == d.r * d.W,
                       "ycc_merge: Yhi is %dx%dx%dx%d beside a %dx%d frame: it must be %dx%dx%dx1 (r = %d on both axes; r is an integer 1..4)", in[0]->n, in[0]->h, in[0]->w,
                       in[0]->c, d.H, d.W, d.N, d.r * d.H, d.r * d.W, d.r);
        SNNHIP_REQUIRE(dims_match(out, d.N, d.r * d.H, d.r * d.W, d.C), "ycc_merge: the output is %dx%dx%dx%d, expected %dx%dx%dx%d", out->n, out->h, out->w, out->c, d.N,
                       d.r * d.H, d.r * d.W, d.C);
        const dim3 grid(static_cast<unsigned>(P.N) * static_cast<unsigned>(P.tilesX) * static_cast<unsigned>(P.tilesY));
        unsigned char* dst = reinterpret_cast<unsigned char*>(out->data);
        dispatch_r_c<3, 4>(d.r, d.C, [&](auto R, auto C) {
            SNNHIP_LAUNCH((ycc_merge_u8_kernel<decltype(R)::value, decltype(C)::value>), grid, dim3(256), 0, ctx->stream, P, bytes_of(in[0]), bytes_of(in[1]), dst);
        });
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }
};

} // namespace
} // namespace snnhip

using namespace snnhip;

extern "C" {

int snnhip_bicubic_taps(int r, float* out, int capacity) {
    int first[4] = {0};
    const int rc = fill_bicubic_taps("bicubic_taps", r, r, SNNHIP_SITING_CENTRE, 0.5, 0.5, out, first, capacity);
    if (rc != SNNHIP_OK) return rc;
    for (int p = 0; p < r; ++p) SNNHIP_REQUIRE(first[p] == phase_first(r, p), "bicubic_taps: phase %d of r = %d starts at %d", p, r, first[p]);
    return SNNHIP_OK;
}

int snnhip_rgb_luma_plan_create(snnhip_ctx* ctx, const snnhip_rgb_luma_desc* desc, snnhip_plan** out) {
    SNNHIP_REQUIRE(ctx && desc && out, "rgb_luma_plan_create: null argument");
    SNNHIP_REQUIRE(desc->N > 0 && desc->H > 0 && desc->W > 0, "rgb_luma desc: bad dims %dx%dx%d", desc->N, desc->H, desc->W);
    SNNHIP_REQUIRE(desc->C == 3 || desc->C == 4, "rgb_luma desc: %d channels (3: RGB8, 4: RGBA8)", desc->C);
    SNNHIP_REQUIRE(matrix_ok(desc->kr, desc->kb), "rgb_luma desc: kr = %g, kb = %g (0 < kr, 0 < kb, kr + kb < 1)", desc->kr, desc->kb);
    auto* plan = new RgbLumaPlan();
    plan->ctx = ctx;
    plan->dtype = SNNHIP_U8;
    plan->rawInput = SNNHIP_U8;
    plan->rawOutput = SNNHIP_U8;
    plan->d = *desc;
    for (int i = 0; i < 4; ++i) plan->inDims[i] = plan->outDims[i] = (&desc->N)[i];
    plan->outDims[3] = 1;
    const double pixels = static_cast<double>(desc->N) * desc->H * desc->W;
    plan->bytes = pixels * (desc->C + 1);
    plan->flops = pixels * 5.0;
    char buf[160];
    snprintf(buf, sizeof(buf), "rgb_luma_u8 c=%d %dx%d kr=%g kb=%g kernel=rgb_luma_u8_kernel", desc->C, desc->H, desc->W, desc->kr, desc->kb);
    plan->desc = buf;
    *out = plan;
    return SNNHIP_OK;
}

int snnhip_ycc_merge_plan_create(snnhip_ctx* ctx, const snnhip_ycc_merge_desc* desc, snnhip_plan** out) {
    SNNHIP_REQUIRE(ctx && desc && out, "ycc_merge_plan_create: null argument");
    SNNHIP_REQUIRE(desc->N > 0 && desc->H > 0 && desc->W > 0, "ycc_merge desc: bad dims %dx%dx%d", desc->N, desc->H, desc->W);
    SNNHIP_REQUIRE(desc->C == 3 || desc->C == 4, "ycc_merge desc: %d channels (3: RGB8, 4: RGBA8)", desc->C);
    SNNHIP_REQUIRE(desc->r >= 1 && desc->r <= 4, "ycc_merge desc: r = %d (an integer 1..4)", desc->r);
    SNNHIP_REQUIRE(matrix_ok(desc->kr, desc->kb), "ycc_merge desc: kr = %g, kb = %g (0 < kr, 0 < kb, kr + kb < 1)", desc->kr, desc->kb);
    const int tilesX = up_div(desc->W, kMergeTileW), tilesY = up_div(desc->H, kMergeTileH);
    const double blocks = static_cast<double>(desc->N) * tilesX * tilesY;
    const double outElems = static_cast<double>(desc->N) * desc->r * desc->H * desc->r * desc->W * desc->C;
    SNNHIP_REQUIRE(blocks < 2147483648.0 && outElems < 9.0e15, "ycc_merge desc: %dx%dx%d at r = %d is too large", desc->N, desc->H, desc->W, desc->r);
    auto* plan = new YccMergePlan();
    plan->ctx = ctx;
    plan->numInputs = 2;
    plan->dtype = SNNHIP_U8; // (input 1, the low-resolution frame, is checked against this; input 0 against rawInput)
    plan->rawInput = SNNHIP_U8;
    plan->rawOutput = SNNHIP_U8;
    plan->d = *desc;
    plan->P = MergeParams{};
    plan->P.N = desc->N;
    plan->P.H = desc->H;
    plan->P.W = desc->W;
    plan->P.tilesX = tilesX;
    plan->P.tilesY = tilesY;
    plan->P.m = make_matrix(desc->kr, desc->kb);
    float taps[16] = {0};
    const int rc = snnhip_bicubic_taps(desc->r, taps, 16);
    if (rc != SNNHIP_OK) {
        delete plan;
        return rc;
    }
    memcpy(plan->P.w, taps, sizeof(taps));
    plan->inDims[0] = desc->N;
    plan->inDims[1] = desc->r * desc->H;
    plan->inDims[2] = desc->r * desc->W;
    plan->inDims[3] = 1;
    plan->outDims[0] = desc->N;
    plan->outDims[1] = desc->r * desc->H;
    plan->outDims[2] = desc->r * desc->W;
    plan->outDims[3] = desc->C;
    const double outPixels = static_cast<double>(desc->N) * desc->r * desc->H * desc->r * desc->W;
    plan->bytes = outPixels * desc->C + outPixels + static_cast<double>(desc->N) * desc->H * desc->W * desc->C; // the output, Yhi, the low-resolution frame: once each
    plan->flops = outPixels * (2.0 * 8.0 * (1.0 + 1.0 / desc->r) + 8.0); // two planes, 4 taps per pass (the horizontal pass shared by r rows), the matrix
    char buf[200];
    snprintf(buf, sizeof(buf), "ycc_merge_u8 r=%d c=%d tile=%dx%d %dx%d -> %dx%d kr=%g kb=%g kernel=ycc_merge_u8_kernel", desc->r, desc->C, kMergeTileH, kMergeTileW, desc->H,
             desc->W, desc->r * desc->H, desc->r * desc->W, desc->kr, desc->kb);
    plan->desc = buf;
    *out = plan;
    return SNNHIP_OK;
}

} // extern "C"
