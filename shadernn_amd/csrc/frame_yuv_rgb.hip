// frame_yuv_rgb.hip -- a 4:2:0 video frame to packed RGB behind a luma-only model (include/snnhip.h: snnhip_yuv_rgb_plan_create /
// snnhip_bicubic_taps_420 / snnhip_yuv_rgb_coefficients).  The reference has no counterpart: core/inc/snn/color.h only names
// YUV layouts, and the libyuv it vendors converts on the CPU.
//
//   yuv_rgb:  Yhi E [N][2rH][2rW][1] + the original CbCr plane E [N][H][W][2] -> E [N][2rH][2rW][C], C = 3 (R, G, B) or 4 (+ A = maxval << shift).
//             v = float(u >> shift); chroma resampled 2r-fold straight to the output luma grid with the separable Keys cubic (a = -0.5, horizontal
//             then vertical, replicate edge, horizontal axis sited), limited or full range, any kr / kb, q = clamp(rint(.), 0, maxval) << shift.
//
// One pass (x2 from 1080p: 8.3 MB of Yhi and 1 MB of chroma in, 24.9 MB of RGB8 out): no upscaled chroma plane is written anywhere.  It
// follows chroma_up_kernel (taps from registers, row march, no LDS, no barrier) with the merge kernel's output side.  One lane owns 4 bytes of a
// chroma row (YuvGeom: two 8-bit or one 16-bit CbCr pixel; the two apron pixels either side are one more load of 4 / 8 bytes each) and the 4r bytes
// of Yhi above them in each of the 2r output rows: one load of r dwords in, C * r dwords out, lanes side by side, so a wave reads and writes one
// contiguous piece of every row.  A wave owns ONE chroma row (five horizontally filtered rows in registers, 2r output rows): two rows per wave
// spend fewer instructions per pixel on the horizontal filter but keep half as many waves on the chip, and measured the same at x2 and slower at x3
// and x4.  As measured, the 8-bit instances are bound by instructions, not by bytes.
// Chroma is staged as v - Coff (exact in fp32), so that neutral chroma filters to exactly 0 whatever the weights' last bits sum to.  The per-phase
// base (-1 or 0) is folded into the tap table on the host as in frame_chroma.hip: five weights over x - 2 .. x + 2, one of them 0, so that every
// register index is a compile-time constant.  Rows whose address is not dword-aligned (the RGB8 pitch 3 * 2rW is 2 mod 4 for odd r and W, and so is
// the 8-bit Yhi pitch), the lane that straddles the right edge and aprons outside the plane take an element path with clamped indices.
//
//   yuv_rgb_planar (snnhip_yuv_rgb_planar_plan_create): the same, with the chroma as two planes E [2N][H][W][1] (I420 / I010).
//             Only the chroma staging differs: the PLANAR branch of yuv_rgb_body; the filter, the matrix and the output side are shared.
#include "frame_yuv_rgb.h"
#include "plan_util.h"
#include "snnhip_internal.h"

namespace snnhip {
namespace {

struct YuvRgbParams {
    int N, H, W; // the CHROMA plane
    int tilesX, tilesY;
    int shift;
    float maxval;
    unsigned alpha; // maxval << shift
    YuvRgbCoeffs m;
    float wh[8][5]; // [phase][offset -2 .. 2] along a row (the desc's siting); rows 2r.. unused
    float wv[8][5]; // ... along a column (centred)
};

// raw[b * 2 + c] = chroma pixel (x0 - 2 + b, channel c) of the row at `row`.  WIDE: three aligned loads -- the lane's own dword and the aprons either
// side (the row is dword-aligned, x0 >= 2 and x0 + CP + 2 <= W); otherwise elements, indices clamped to [0, W - 1] (x0 < W)
template <int R, typename E, bool WIDE>
__device__ __forceinline__ void yuv_load_chroma(const E* __restrict__ row, int x0, int W, unsigned* raw) {
    using G = YuvGeom<R, E>;
    if constexpr (WIDE) {
        constexpr int AW = 2 * 2 * G::ES / 4; // dwords of one apron
        const E* p = row + static_cast<size_t>(x0) * 2;
        unsigned w[2 * AW + 1]; // left apron, the lane's own dword, right apron: NB elements in a row
        load_words<AW>(p - 4, w);
        load_words<1>(p, w + AW);
        load_words<AW>(p + 2 * G::CP, w + AW + 1);
#pragma unroll
        for (int e = 0; e < G::NB; ++e) raw[e] = frame_elem<E>(w, e);
    } else {
#pragma unroll
        for (int e = 0; e < G::NB; ++e) {
            const int px = min(max(x0 - 2 + e / 2, 0), W - 1);
            raw[e] = row[static_cast<size_t>(px) * 2 + e % 2];
        }
    }
}

// one staged chroma row, as sample - Coff, resampled to the lane's output columns: output pixel j reads chroma pixel j / 2r at phase j % 2r
template <int R, typename E>
__device__ __forceinline__ void yuv_hfilter(const YuvRgbParams& P, const unsigned* raw, float* h) {
    using G = YuvGeom<R, E>;
    float v[G::NB];
#pragma unroll
    for (int e = 0; e < G::NB; ++e) v[e] = static_cast<float>(raw[e] >> P.shift) - P.m.coff;
    frame_hfilter<G::R2, 2, G::CP>(P.wh, v, h);
}

// the lane's OPX pixels of one output row: u = its dwords of Yhi, w = its C * r dwords of output
template <int R, int C, typename E>
__device__ __forceinline__ void yuv_row(const YuvRgbParams& P, const float (&h)[5][YuvGeom<R, E>::OPX * 2], int q, const unsigned* u, unsigned* w) {
    using G = YuvGeom<R, E>;
#pragma unroll
    for (int k = 0; k < G::YW * C; ++k) w[k] = 0u;
#pragma unroll
    for (int j = 0; j < G::OPX; ++j) {
        float cb = P.wv[q][0] * h[0][j * 2], cr = P.wv[q][0] * h[0][j * 2 + 1];
#pragma unroll
        for (int k = 1; k < 5; ++k) {
            cb += P.wv[q][k] * h[k][j * 2];
            cr += P.wv[q][k] * h[k][j * 2 + 1];
        }
        const float yl = P.m.cy * (static_cast<float>(frame_elem<E>(u, j) >> P.shift) - P.m.yoff);
        unsigned e[4];
        e[0] = quantize_frame(yl + P.m.crv * cr, P.maxval) << P.shift;
        e[1] = quantize_frame(yl - (P.m.cgv * cr + P.m.cgu * cb), P.maxval) << P.shift;
        e[2] = quantize_frame(yl + P.m.cbu * cb, P.maxval) << P.shift;
        e[3] = P.alpha;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int i = j * C + c;
            w[i / G::PER] |= e[c] << (8 * G::ES * (i % G::PER));
        }
    }
}

// ---- planar chroma (I420 / I010): E [2N][H][W][1], plane 2n = Cb, 2n + 1 = Cr of image n.  The lane keeps the geometry of the interleaved kernel
// (CP chroma pixels, the same raw[NB] and h[5][OPX * 2]): its CP + 4 staged samples of ONE component are 6 bytes (8-bit) or 10 bytes (16-bit) that
// start 2 (x0 - 2) * ES / 2 bytes into the row -- a multiple of 2.  The PW dwords from the dword at or below that byte cover them (2 + 6 <= 8,
// 2 + 10 <= 12): one load per plane and row, ten per lane where the interleaved kernel issues fifteen, shifted right by 0 or 16 bits.  Widening the
// lane to a dword of each plane instead would double h to 320 floats at r = 4.

template <typename E>
struct YuvPlanarGeom {
    static constexpr int ES = static_cast<int>(sizeof(E));
    static constexpr int NS = 4 / (2 * ES) + 4;            // staged samples of one component per lane and row (YuvGeom::NB / 2)
    static constexpr int PW = (NS * ES + 2 + 3) / 4;        // dwords that cover them from the dword below their first byte
};

// whether the PW dwords of a lane lie inside a row of W samples (x0 < W): the first at or below sample x0 - 2, the last ending at or before the row's end
template <typename E>
__device__ __forceinline__ bool yuv_planar_inside(int x0, int W) {
    using Q = YuvPlanarGeom<E>;
    if (x0 < 2) return false;
    const size_t a = static_cast<size_t>(x0 - 2) * Q::ES;
    return (a & ~static_cast<size_t>(3)) + 4 * Q::PW <= static_cast<size_t>(W) * Q::ES;
}

// raw[b * 2 + c] = sample x0 - 2 + b of component c's row at `row`.  WIDE: one load of PW dwords (the row is dword-aligned and yuv_planar_inside);
// otherwise elements, indices clamped to [0, W - 1]
template <typename E, bool WIDE>
__device__ __forceinline__ void yuv_load_plane(const E* __restrict__ row, int x0, int W, int c, unsigned* raw) {
    using Q = YuvPlanarGeom<E>;
    if constexpr (WIDE) {
        const size_t a = static_cast<size_t>(x0 - 2) * Q::ES;
        const unsigned sh = static_cast<unsigned>(a & 3) * 8u; // 0 or 16
        unsigned w[Q::PW], s[Q::PW];
        load_words<Q::PW>(reinterpret_cast<const unsigned char*>(row) + (a & ~static_cast<size_t>(3)), w);
#pragma unroll
        for (int k = 0; k + 1 < Q::PW; ++k) s[k] = static_cast<unsigned>(((static_cast<unsigned long long>(w[k + 1]) << 32) | w[k]) >> sh);
        s[Q::PW - 1] = w[Q::PW - 1] >> sh;
#pragma unroll
        for (int b = 0; b < Q::NS; ++b) raw[b * 2 + c] = frame_elem<E>(s, b);
    } else {
#pragma unroll
        for (int b = 0; b < Q::NS; ++b) raw[b * 2 + c] = row[min(max(x0 - 2 + b, 0), W - 1)];
    }
}

// PLANAR (snnhip_yuv_rgb_planar_plan_create): `cbcr` is the planar chroma tensor [2N][H][W][1].  Only the staging of the five chroma rows differs; the
// lane, raw[], h[][], the filter and the whole output side are the interleaved kernel's
template <int R, int C, typename E, bool PLANAR = false>
__device__ __forceinline__ void yuv_rgb_body(const YuvRgbParams& P, const E* __restrict__ yhi, const E* __restrict__ cbcr, E* __restrict__ out) {
    using G = YuvGeom<R, E>;
    constexpr int OD = G::YW * C; // dwords of output per lane and output row
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = P.H, W = P.W;
    const size_t OH = static_cast<size_t>(G::R2) * H, OW = static_cast<size_t>(G::R2) * W;
    const FrameTile tile = frame_tile(blockIdx.x, P.tilesX, P.tilesY);
    const size_t n = tile.n;
    const int x0 = (tile.tx * 64 + lane) * G::CP;
    const int y = tile.ty * G::TILE_H + wave;
    if (x0 >= W || y >= H) return; // (no barrier anywhere below)
    float h[5][G::OPX * 2];
    if constexpr (PLANAR) {
        static_assert(YuvPlanarGeom<E>::NS * 2 == G::NB, "the planar staging fills the interleaved kernel's raw[]");
        const size_t planeElems = static_cast<size_t>(H) * W;
        const E* cb = cbcr + 2 * n * planeElems;
        const E* cr = cb + planeElems; // H * W * sizeof(E) bytes behind Cb: aligned as Cb is only if that is a multiple of 4
        // chroma rows y - 2 .. y + 2 (clamped to the plane) of both planes.  With a pitch that is a multiple of 4 bytes and both planes on a dword every
        // row is: one decision for the wave, the ten loads of an interior lane in flight before the first is used.  Otherwise each row of each plane
        // decides for itself (an odd W puts every other 16-bit row and every fourth 8-bit row on a dword)
        const bool inside = yuv_planar_inside<E>(x0, W);
        const bool planesAligned = ((reinterpret_cast<size_t>(cb) | reinterpret_cast<size_t>(cr)) & 3) == 0 && (static_cast<size_t>(W) * G::ES) % 4 == 0;
        if (planesAligned && inside) {
            unsigned raw[5][G::NB];
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const size_t ro = static_cast<size_t>(min(max(y - 2 + i, 0), H - 1)) * W;
                yuv_load_plane<E, true>(cb + ro, x0, W, 0, raw[i]);
                yuv_load_plane<E, true>(cr + ro, x0, W, 1, raw[i]);
            }
#pragma unroll
            for (int i = 0; i < 5; ++i) yuv_hfilter<R, E>(P, raw[i], h[i]);
        } else {
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const size_t ro = static_cast<size_t>(min(max(y - 2 + i, 0), H - 1)) * W;
                unsigned raw[G::NB];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const E* row = (c ? cr : cb) + ro;
                    if (inside && (reinterpret_cast<size_t>(row) & 3) == 0) yuv_load_plane<E, true>(row, x0, W, c, raw);
                    else yuv_load_plane<E, false>(row, x0, W, c, raw);
                }
                yuv_hfilter<R, E>(P, raw, h[i]);
            }
        }
    } else {
        const E* plane = cbcr + n * H * W * 2;

        // chroma rows y - 2 .. y + 2 (clamped to the plane), resampled to the lane's output columns.  Whether a row starts on a dword is the same for
        // every row of a plane whose pitch is a multiple of 4 bytes: one decision for the wave, and all fifteen loads of an interior lane are in flight
        // before the first is used
        const bool chromaAligned = (reinterpret_cast<size_t>(plane) & 3) == 0 && (static_cast<size_t>(W) * 2 * G::ES) % 4 == 0;
        if (chromaAligned && x0 >= 2 && x0 + G::CP + 2 <= W) {
            unsigned raw[5][G::NB];
#pragma unroll
            for (int i = 0; i < 5; ++i) yuv_load_chroma<R, E, true>(plane + static_cast<size_t>(min(max(y - 2 + i, 0), H - 1)) * W * 2, x0, W, raw[i]);
#pragma unroll
            for (int i = 0; i < 5; ++i) yuv_hfilter<R, E>(P, raw[i], h[i]);
        } else {
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                unsigned raw[G::NB];
                yuv_load_chroma<R, E, false>(plane + static_cast<size_t>(min(max(y - 2 + i, 0), H - 1)) * W * 2, x0, W, raw);
                yuv_hfilter<R, E>(P, raw, h[i]);
            }
        }
    }

    // the 2r output rows under chroma row y.  The lane's piece of a row starts a multiple of 4 bytes into it, so with dword-aligned bases and pitches
    // (again one decision for the wave) a lane that lies inside the frame loads r dwords of Yhi and stores C * r dwords per row: 2r independent loads
    const size_t pix0 = (n * OH + static_cast<size_t>(G::R2) * y) * OW + static_cast<size_t>(G::R2) * x0;
    const bool full = x0 + G::CP <= W;
    const bool rowsAligned = ((reinterpret_cast<size_t>(yhi) | reinterpret_cast<size_t>(out)) & 3) == 0 && (OW * G::ES) % 4 == 0 && (OW * C * G::ES) % 4 == 0;
    if (rowsAligned && full) {
        unsigned u[G::R2][G::YW];
#pragma unroll
        for (int q = 0; q < G::R2; ++q) load_words<G::YW>(yhi + pix0 + q * OW, u[q]);
#pragma unroll
        for (int q = 0; q < G::R2; ++q) {
            unsigned w[OD];
            yuv_row<R, C, E>(P, h, q, u[q], w);
            store_words<OD>(out + (pix0 + q * OW) * C, w);
        }
    } else { // a row that does not start on a dword, or the lane that straddles the right edge: elements
        const int valid = min(G::CP, W - x0) * G::R2; // output pixels of this lane inside the frame
#pragma unroll
        for (int q = 0; q < G::R2; ++q) {
            const E* ysrc = yhi + pix0 + q * OW;
            E* dst = out + (pix0 + q * OW) * C;
            unsigned u[G::YW], w[OD];
#pragma unroll
            for (int k = 0; k < G::YW; ++k) u[k] = 0u;
#pragma unroll
            for (int j = 0; j < G::OPX; ++j)
                if (j < valid) u[j / G::PER] |= static_cast<unsigned>(ysrc[j]) << (8 * G::ES * (j % G::PER));
            yuv_row<R, C, E>(P, h, q, u, w);
#pragma unroll
            for (int i = 0; i < G::OPX * C; ++i)
                if (i < valid * C) dst[i] = static_cast<E>(frame_elem<E>(w, i));
        }
    }
}

template <int R, int C, typename E>
__global__ __launch_bounds__(256) void yuv_rgb_kernel(YuvRgbParams P, const E* __restrict__ yhi, const E* __restrict__ cbcr, E* __restrict__ out) {
    yuv_rgb_body<R, C, E>(P, yhi, cbcr, out);
}

template <int R, int C, typename E>
__global__ __launch_bounds__(256) void yuv_rgb_planar_kernel(YuvRgbParams P, const E* __restrict__ yhi, const E* __restrict__ chroma, E* __restrict__ out) {
    yuv_rgb_body<R, C, E, true>(P, yhi, chroma, out);
}

struct YuvRgbPlan : snnhip_plan {
    snnhip_yuv_rgb_desc d;
    YuvRgbParams P;
    bool planar = false; // the chroma input is [2N][H][W][1] (snnhip_yuv_rgb_planar_plan_create)

    template <typename E>
    void launch(const snnhip_tensor* y, const snnhip_tensor* c, snnhip_tensor* out) {
        const dim3 grid(static_cast<unsigned>(P.N) * static_cast<unsigned>(P.tilesX) * static_cast<unsigned>(P.tilesY));
        const E* ysrc = reinterpret_cast<const E*>(y->data);
        const E* csrc = reinterpret_cast<const E*>(c->data);
        E* dst = reinterpret_cast<E*>(out->data);
        dispatch_r_c<3, 4>(d.r, d.C, [&](auto R, auto C) {
            if (planar) SNNHIP_LAUNCH((yuv_rgb_planar_kernel<decltype(R)::value, decltype(C)::value, E>), grid, dim3(256), 0, ctx->stream, P, ysrc, csrc, dst);
            else SNNHIP_LAUNCH((yuv_rgb_kernel<decltype(R)::value, decltype(C)::value, E>), grid, dim3(256), 0, ctx->stream, P, ysrc, csrc, dst);
        });
    }

    int run_planar(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) {
        const int R2 = 2 * d.r;
        SNNHIP_REQUIRE(nIn == 2, "yuv_rgb_planar: expects 2 inputs (Yhi, the planar chroma tensor), got %d", nIn);
        SNNHIP_REQUIRE(in[0]->dtype == d.dtype && in[1]->dtype == d.dtype && out->dtype == d.dtype, "yuv_rgb_planar: every tensor must have dtype %d, got %d, %d and %d", d.dtype,
                       in[0]->dtype, in[1]->dtype, out->dtype);
        SNNHIP_REQUIRE(dims_match(in[1], 2 * d.N, d.H, d.W, 1),
                       "yuv_rgb_planar: the chroma tensor is %dx%dx%dx%d, the plan was built for %dx%dx%dx1 ([2N][H][W][1]: plane 2n is Cb, 2n + 1 Cr of image n)", in[1]->n,
                       in[1]->h, in[1]->w, in[1]->c, 2 * d.N, d.H, d.W);
        SNNHIP_REQUIRE(dims_match(in[0], d.N, R2 * d.H, R2 * d.W, 1), "yuv_rgb_planar: Yhi is %dx%dx%dx%d beside %dx%d chroma planes: it must be %dx%dx%dx1 (2r = %d times a plane)",
                       in[0]->n, in[0]->h, in[0]->w, in[0]->c, d.H, d.W, d.N, R2 * d.H, R2 * d.W, R2);
        SNNHIP_REQUIRE(dims_match(out, d.N, R2 * d.H, R2 * d.W, d.C), "yuv_rgb_planar: the output is %dx%dx%dx%d, expected %dx%dx%dx%d (2r = %d times a chroma plane)", out->n,
                       out->h, out->w, out->c, d.N, R2 * d.H, R2 * d.W, d.C, R2);
        if (d.dtype == SNNHIP_U8) launch<unsigned char>(in[0], in[1], out);
        else launch<unsigned short>(in[0], in[1], out);
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }

    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        if (planar) return run_planar(in, nIn, out);
        const int R2 = 2 * d.r;
        SNNHIP_REQUIRE(nIn == 2, "yuv_rgb: expects 2 inputs (Yhi, the chroma plane), got %d", nIn);
        SNNHIP_REQUIRE(in[0]->dtype == d.dtype && in[1]->dtype == d.dtype && out->dtype == d.dtype, "yuv_rgb: every tensor must have dtype %d, got %d, %d and %d", d.dtype,
                       in[0]->dtype, in[1]->dtype, out->dtype);
        SNNHIP_REQUIRE(dims_match(in[1], d.N, d.H, d.W, 2), "yuv_rgb: the chroma plane is %dx%dx%dx%d, the plan was built for %dx%dx%dx2", in[1]->n, in[1]->h, in[1]->w, in[1]->c,
                       d.N, d.H, d.W);
        SNNHIP_REQUIRE(dims_match(in[0], d.N, R2 * d.H, R2 * d.W, 1), "yuv_rgb: Yhi is %dx%dx%dx%d beside a %dx%d chroma plane: it must be %dx%dx%dx1 (2r = %d times the plane)",
                       in[0]->n, in[0]->h, in[0]->w, in[0]->c, d.H, d.W, d.N, R2 * d.H, R2 * d.W, R2);
        SNNHIP_REQUIRE(dims_match(out, d.N, R2 * d.H, R2 * d.W, d.C), "yuv_rgb: the output is %dx%dx%dx%d, expected %dx%dx%dx%d (2r = %d times the chroma plane)", out->n, out->h,
                       out->w, out->c, d.N, R2 * d.H, R2 * d.W, d.C, R2);
        if (d.dtype == SNNHIP_U8) launch<unsigned char>(in[0], in[1], out);
        else launch<unsigned short>(in[0], in[1], out);
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }
};

} // namespace
} // namespace snnhip

using namespace snnhip;

extern "C" {

int snnhip_bicubic_taps_420(int r, int siting, float* weights, int* base, int capacity) {
    // straight to the output luma grid, 2r-fold (bicubic_phase_420): lead = 0.5 whatever the siting
    return fill_bicubic_taps("bicubic_taps_420", r, 2 * r, siting, 0.5, siting_offset(siting), weights, base, capacity);
}

int snnhip_yuv_rgb_coefficients(int maxval, int range, float kr, float kb, float* out, int capacity) {
    SNNHIP_REQUIRE(out, "yuv_rgb_coefficients: null argument");
    SNNHIP_REQUIRE(capacity >= 7, "yuv_rgb_coefficients: room for %d floats, 7 needed", capacity);
    SNNHIP_REQUIRE(maxval >= 255 && maxval <= 65535 && (maxval + 1) % 256 == 0, "yuv_rgb_coefficients: maxval %d (maxval + 1 must be a multiple of 256)", maxval);
    SNNHIP_REQUIRE(range == SNNHIP_RANGE_LIMITED || range == SNNHIP_RANGE_FULL, "yuv_rgb_coefficients: range %d (SNNHIP_RANGE_LIMITED or SNNHIP_RANGE_FULL)", range);
    SNNHIP_REQUIRE(matrix_ok(kr, kb), "yuv_rgb_coefficients: kr = %g, kb = %g (0 < kr, 0 < kb, kr + kb < 1)", kr, kb);
    const YuvRgbCoeffs c = yuv_rgb_coeffs(maxval, range, kr, kb);
    out[0] = c.yoff, out[1] = c.coff, out[2] = c.cy, out[3] = c.crv, out[4] = c.cbu, out[5] = c.cgv, out[6] = c.cgu;
    return SNNHIP_OK;
}

// snnhip_yuv_rgb_plan_create and snnhip_yuv_rgb_planar_plan_create: one desc, one set of checks, tables and coefficients
static int yuv_rgb_plan_make(snnhip_ctx* ctx, const snnhip_yuv_rgb_desc* desc, snnhip_plan** out, bool planar) {
    SNNHIP_REQUIRE(ctx && desc && out, "%s: null argument", planar ? "yuv_rgb_planar_plan_create" : "yuv_rgb_plan_create");
    SNNHIP_REQUIRE(desc->N > 0 && desc->H > 0 && desc->W > 0, "yuv_rgb desc: bad dims %dx%dx%d", desc->N, desc->H, desc->W);
    SNNHIP_REQUIRE(desc->C == 3 || desc->C == 4, "yuv_rgb desc: %d channels (3: RGB, 4: RGBA)", desc->C);
    SNNHIP_REQUIRE(desc->r >= 1 && desc->r <= 4, "yuv_rgb desc: r = %d (an integer 1..4)", desc->r);
    int bits = 0;
    const int fmt = check_sample_format("yuv_rgb desc", "frames", desc->dtype, desc->siting, desc->shift, desc->maxval, &bits);
    if (fmt != SNNHIP_OK) return fmt;
    SNNHIP_REQUIRE(desc->range == SNNHIP_RANGE_LIMITED || desc->range == SNNHIP_RANGE_FULL, "yuv_rgb desc: range %d (SNNHIP_RANGE_LIMITED or SNNHIP_RANGE_FULL)", desc->range);
    SNNHIP_REQUIRE((desc->maxval + 1) % 256 == 0, "yuv_rgb desc: maxval %d: maxval + 1 must be a multiple of 256 (the offsets 16k, 128k of the matrix are integers)", desc->maxval);
    SNNHIP_REQUIRE(matrix_ok(desc->kr, desc->kb), "yuv_rgb desc: kr = %g, kb = %g (0 < kr, 0 < kb, kr + kb < 1)", desc->kr, desc->kb);
    int th = 0, tw = 0;
    yuv_rgb_tile(bits / 8, &th, &tw);
    const int R2 = 2 * desc->r;
    const int tilesX = up_div(desc->W, tw), tilesY = up_div(desc->H, th);
    const double blocks = static_cast<double>(desc->N) * tilesX * tilesY;
    const double chromaElems = static_cast<double>(desc->N) * desc->H * desc->W * 2.0;
    const double outPixels = static_cast<double>(desc->N) * R2 * desc->H * R2 * desc->W;
    SNNHIP_REQUIRE(blocks < 2147483648.0 && outPixels * desc->C < 9.0e15 && static_cast<double>(R2) * desc->H < 2147483648.0 && static_cast<double>(R2) * desc->W < 2147483648.0,
                   "yuv_rgb desc: %dx%dx%d at r = %d is too large", desc->N, desc->H, desc->W, desc->r);
    float wh[32] = {0}, wv[32] = {0};
    int bh[8] = {0}, bv[8] = {0};
    int rc = snnhip_bicubic_taps_420(desc->r, desc->siting, wh, bh, 32);
    if (rc == SNNHIP_OK) rc = snnhip_bicubic_taps_420(desc->r, SNNHIP_SITING_CENTRE, wv, bv, 32);
    if (rc != SNNHIP_OK) return rc;
    auto* plan = new YuvRgbPlan();
    plan->ctx = ctx;
    plan->numInputs = 2;
    plan->dtype = desc->dtype; // (input 1, the chroma plane, is checked against this; input 0 against rawInput)
    plan->rawInput = desc->dtype;
    plan->rawOutput = desc->dtype;
    plan->d = *desc;
    plan->planar = planar;
    plan->P = YuvRgbParams{};
    plan->P.N = desc->N;
    plan->P.H = desc->H;
    plan->P.W = desc->W;
    plan->P.tilesX = tilesX;
    plan->P.tilesY = tilesY;
    plan->P.shift = desc->shift;
    plan->P.maxval = static_cast<float>(desc->maxval);
    plan->P.alpha = static_cast<unsigned>(desc->maxval) << desc->shift;
    plan->P.m = yuv_rgb_coeffs(desc->maxval, desc->range, desc->kr, desc->kb);
    widen_taps(R2, wh, bh, plan->P.wh);
    widen_taps(R2, wv, bv, plan->P.wv);
    plan->inDims[0] = plan->outDims[0] = desc->N;
    plan->inDims[1] = plan->outDims[1] = R2 * desc->H;
    plan->inDims[2] = plan->outDims[2] = R2 * desc->W;
    plan->inDims[3] = 1;
    plan->outDims[3] = desc->C;
    plan->bytes = (outPixels + chromaElems + outPixels * desc->C) * (bits / 8); // Yhi, the chroma plane and the output: once each
    plan->flops = outPixels * (2.0 * 2.0 * 4.0 * (1.0 + 1.0 / R2) + 12.0);        // two planes, 4 taps per pass (the horizontal pass shared by 2r rows), the matrix
    char buf[280];
    snprintf(buf, sizeof(buf), "%s%d r=%d c=%d siting=%s range=%s tile=%dx%d %dx%d -> %dx%d maxval=%d shift=%d kr=%g kb=%g kernel=%s", planar ? "yuv_rgb_planar_u" : "yuv_rgb_u", bits, desc->r, desc->C,
             desc->siting == SNNHIP_SITING_LEFT ? "left" : "centre", desc->range == SNNHIP_RANGE_LIMITED ? "limited" : "full", th, tw, desc->H, desc->W, R2 * desc->H,
             R2 * desc->W, desc->maxval, desc->shift, desc->kr, desc->kb, planar ? "yuv_rgb_planar_kernel" : "yuv_rgb_kernel");
    plan->desc = buf;
    *out = plan;
    return SNNHIP_OK;
}

int snnhip_yuv_rgb_plan_create(snnhip_ctx* ctx, const snnhip_yuv_rgb_desc* desc, snnhip_plan** out) { return yuv_rgb_plan_make(ctx, desc, out, false); }

int snnhip_yuv_rgb_planar_plan_create(snnhip_ctx* ctx, const snnhip_yuv_rgb_desc* desc, snnhip_plan** out) { return yuv_rgb_plan_make(ctx, desc, out, true); }

} // extern "C"
