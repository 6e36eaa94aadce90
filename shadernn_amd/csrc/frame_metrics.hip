// frame_metrics.hip -- PSNR and SSIM between two frames on the device (include/snnhip.h: snnhip_frame_metrics_plan_create / _read / _psnr; DESIGN.md
// section 4.22).  The reference ships a host-side comparison script only (tools/misc/imageComparison.py); nothing of it is restated here: the definition
// is the integer-moment SSIM on 8x8 windows with a 4-pixel step that x264 and ffmpeg's ssim filter compute, stated once in include/snnhip.h.
//
//   frame_metrics_tile_kernel<T, C>:  a block owns a tile of kMetricsTileH x kMetricsTileW pixels (frame_metrics.h) of one image, one 4x4 block per
//       thread, and reads one more block row and column so that every window anchored in the tile is complete.  A thread loads its 4x4 block of both
//       frames (four rows of 4 * C samples each, 4 / 8 / 16-byte loads where the rows are aligned, element loads with clamped extent otherwise), forms
//       the exact integer moments s1 = sum a, s2 = sum b, ss = sum (a^2 + b^2), s12 = sum a b per channel -- 8-bit samples as v_dot4_u32_u8 products of
//       the loaded dwords against byte masks, 16-bit samples in 64-bit integers -- and puts them into LDS.  The block's share of the squared error comes
//       from the same moments, sum (a - b)^2 = ss - 2 s12, the ragged right and bottom pixels included (they are loaded with zeros past the frame's
//       edge in BOTH frames).  After one barrier every thread sums the 2x2 group of blocks under its window and evaluates t in fp64 without
//       contraction (every product in it is an exact integer below 2^53, so equal frames give exactly 1).  The block adds its t's and squared errors
//       in a fixed order (a shuffle tree per wave, the four waves in index order) and writes ONE partial per channel.
//   frame_metrics_fold_kernel:        one block per (image, channel) adds that pair's partials in a fixed order and writes the result row and
//       {psnr_db, ssim} as fp32.
//
// No atomics and no memset: every partial and every row is written by exactly one thread on every run, so a result is bit-identical from run to run and
// the two launches can be recorded in a graph.
#include <cmath>

#include "frame_metrics.h"
#include "plan_util.h"
#include "snnhip_internal.h"

namespace snnhip {
namespace {

struct MetricsParams {
    int N, H, W;
    int bh, bw; // whole 4x4 blocks per column / row: H >> 2, W >> 2
    int tilesX, tilesY;
    int shift;
    double c1, c2;
};

template <typename T>
struct MetricsMoment;
template <>
struct MetricsMoment<unsigned char> { // 16 * 2 * 255^2 per block, four blocks per window: 32 bits are enough
    using type = unsigned;
};
template <>
struct MetricsMoment<unsigned short> { // 16 * 65535^2 > 2^32
    using type = unsigned long long;
};

// the bytes of dword k of a row of interleaved 8-bit pixels that belong to channel c
__host__ __device__ constexpr unsigned metrics_byte_mask(int c, int k, int C) {
    unsigned m = 0;
    for (int j = 0; j < 4; ++j)
        if ((4 * k + j) % C == c) m |= 0xFFu << (8 * j);
    return m;
}

// DW dwords from an address aligned to 16, 8 or 4 bytes, whichever is the widest that divides the row
template <int DW>
__device__ __forceinline__ void metrics_load_row(const unsigned char* p, unsigned* w) {
    constexpr int V = DW % 4 == 0 ? 4 : DW % 2 == 0 ? 2 : 1;
#pragma unroll
    for (int k = 0; k < DW; k += V) {
        if constexpr (V == 4) {
            const uint4 q = *reinterpret_cast<const uint4*>(p + 4 * k);
            w[k] = q.x, w[k + 1] = q.y, w[k + 2] = q.z, w[k + 3] = q.w;
        } else if constexpr (V == 2) {
            const uint2 q = *reinterpret_cast<const uint2*>(p + 4 * k);
            w[k] = q.x, w[k + 1] = q.y;
        } else {
            w[k] = *reinterpret_cast<const unsigned*>(p + 4 * k);
        }
    }
}

// the same row from element loads, samples at or past column W read as 0
template <typename T, int C>
__device__ __forceinline__ void metrics_load_row_elems(const T* __restrict__ row, int x0, int W, unsigned* w) {
    constexpr int ES = sizeof(T), PER = 4 / ES;
#pragma unroll
    for (int k = 0; k < C * ES; ++k) w[k] = 0u;
#pragma unroll
    for (int e = 0; e < 4 * C; ++e) {
        const int x = x0 + e / C;
        const unsigned v = x < W ? static_cast<unsigned>(row[static_cast<size_t>(x) * C + e % C]) : 0u;
        w[e / PER] |= v << (8 * ES * (e % PER));
    }
}

// one row of 4 pixels of both frames into the per-channel moments
template <int C>
__device__ __forceinline__ void metrics_row_moments(const unsigned* wa, const unsigned* wb, int, unsigned* s1, unsigned* s2, unsigned* ss, unsigned* s12, unsigned char) {
#pragma unroll
    for (int k = 0; k < C; ++k) // C dwords of 8-bit samples
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const unsigned m = metrics_byte_mask(c, k, C);
            const unsigned am = wa[k] & m, bm = wb[k] & m;
            s1[c] = __builtin_amdgcn_udot4(wa[k], m & 0x01010101u, s1[c], false);
            s2[c] = __builtin_amdgcn_udot4(wb[k], m & 0x01010101u, s2[c], false);
            ss[c] = __builtin_amdgcn_udot4(am, wa[k], ss[c], false);
            ss[c] = __builtin_amdgcn_udot4(bm, wb[k], ss[c], false);
            s12[c] = __builtin_amdgcn_udot4(am, wb[k], s12[c], false);
        }
}
template <int C>
__device__ __forceinline__ void metrics_row_moments(const unsigned* wa, const unsigned* wb, int shift, unsigned* s1, unsigned* s2, unsigned long long* ss,
                                                    unsigned long long* s12, unsigned short) {
#pragma unroll
    for (int e = 0; e < 4 * C; ++e) {
        const unsigned a = ((wa[e / 2] >> (16 * (e % 2))) & 0xFFFFu) >> shift;
        const unsigned b = ((wb[e / 2] >> (16 * (e % 2))) & 0xFFFFu) >> shift;
        const int c = e % C;
        s1[c] += a; // 16 * 65535 per block
        s2[c] += b;
        ss[c] += static_cast<unsigned long long>(a * a) + static_cast<unsigned long long>(b * b); // 65535^2 < 2^32: each product is exact in 32 bits
        s12[c] += static_cast<unsigned long long>(a * b);
    }
}

// t of one window from its exact integer moments (all below 2^53 in double).  Contraction is off: every product below is an exact integer, so fusing
// would change nothing today, and the statement "equal frames give exactly 1" should not rest on that.
__device__ __forceinline__ double metrics_window_t(double s1, double s2, double ss, double s12, double c1, double c2) {
#pragma clang fp contract(off)
    const double vars = 64.0 * ss - s1 * s1 - s2 * s2;
    const double covar = 64.0 * s12 - s1 * s2;
    return ((2.0 * s1 * s2 + c1) * (2.0 * covar + c2)) / ((s1 * s1 + s2 * s2 + c1) * (vars + c2));
}

template <typename T, int C>
__global__ __launch_bounds__(kMetricsThreads) void frame_metrics_tile_kernel(MetricsParams P, const T* __restrict__ a, const T* __restrict__ b,
                                                                            MetricsPartial* __restrict__ part) {
    using M = typename MetricsMoment<T>::type;
    constexpr int ES = sizeof(T), DW = C * ES; // dwords in a row of 4 pixels
    constexpr int VECB = DW % 4 == 0 ? 16 : DW % 2 == 0 ? 8 : 4;
    __shared__ unsigned sS1[C][kMetricsPositions], sS2[C][kMetricsPositions];
    __shared__ M sSS[C][kMetricsPositions], sS12[C][kMetricsPositions];
    __shared__ double sWaveT[C][kMetricsThreads / 64];
    __shared__ unsigned long long sWaveE[C][kMetricsThreads / 64];

    const int tid = threadIdx.x;
    const int tiles = P.tilesX * P.tilesY;
    const int n = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int ty = tile / P.tilesX, tx = tile % P.tilesX;
    const int H = P.H, W = P.W;
    const size_t pitch = static_cast<size_t>(W) * C; // elements
    const T* pa = a + static_cast<size_t>(n) * H * pitch;
    const T* pb = b + static_cast<size_t>(n) * H * pitch;
    // every row of both images starts on a multiple of the load width (uniform over the block)
    const bool aligned = ((reinterpret_cast<size_t>(pa) | reinterpret_cast<size_t>(pb)) & (VECB - 1)) == 0 && (pitch * ES) % VECB == 0;

    unsigned long long sse[C];
#pragma unroll
    for (int c = 0; c < C; ++c) sse[c] = 0ull;

    // positions 0 .. 255: the tile's own blocks, one per thread; 256 .. 296: the halo (the column to the right, then the row below)
    for (int p = tid; p < kMetricsPositions; p += kMetricsThreads) {
        const bool owned = p < kMetricsThreads;
        int iy, ix;
        if (owned) {
            iy = p / kMetricsBlocksX, ix = p % kMetricsBlocksX;
        } else if (p - kMetricsThreads < kMetricsBlocksY) {
            iy = p - kMetricsThreads, ix = kMetricsBlocksX;
        } else {
            iy = kMetricsBlocksY, ix = p - kMetricsThreads - kMetricsBlocksY;
        }
        const int gy = ty * kMetricsBlocksY + iy, gx = tx * kMetricsBlocksX + ix;
        const bool full = gy < P.bh && gx < P.bw;            // a whole block inside the frame: takes part in SSIM
        const bool ragged = 4 * gy < H && 4 * gx < W && !full; // cut by the right or bottom edge: squared error only
        if (!full && !(owned && ragged)) continue;

        unsigned wa[4][DW], wb[4][DW];
        const int x0 = 4 * gx;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int y = 4 * gy + r;
            if (full && aligned) {
                const size_t off = (static_cast<size_t>(y) * pitch + static_cast<size_t>(x0) * C) * ES;
                metrics_load_row<DW>(reinterpret_cast<const unsigned char*>(pa) + off, wa[r]);
                metrics_load_row<DW>(reinterpret_cast<const unsigned char*>(pb) + off, wb[r]);
            } else if (y < H) {
                metrics_load_row_elems<T, C>(pa + static_cast<size_t>(y) * pitch, x0, W, wa[r]);
                metrics_load_row_elems<T, C>(pb + static_cast<size_t>(y) * pitch, x0, W, wb[r]);
            } else {
#pragma unroll
                for (int k = 0; k < DW; ++k) wa[r][k] = wb[r][k] = 0u;
            }
        }
        unsigned s1[C], s2[C];
        M ss[C], s12[C];
#pragma unroll
        for (int c = 0; c < C; ++c) s1[c] = 0u, s2[c] = 0u, ss[c] = 0, s12[c] = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) metrics_row_moments<C>(wa[r], wb[r], P.shift, s1, s2, ss, s12, T{});
        const int slot = iy * kMetricsHaloX + ix;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (full) sS1[c][slot] = s1[c], sS2[c][slot] = s2[c], sSS[c][slot] = ss[c], sS12[c][slot] = s12[c];
            if (owned) sse[c] += static_cast<unsigned long long>(ss[c]) - 2ull * static_cast<unsigned long long>(s12[c]); // sum (a - b)^2
        }
    }
    __syncthreads();

    // the window anchored at this thread's own block: that block and its right, lower and lower-right neighbours
    const int iy = tid / kMetricsBlocksX, ix = tid % kMetricsBlocksX;
    const int gy = ty * kMetricsBlocksY + iy, gx = tx * kMetricsBlocksX + ix;
    const bool window = gy + 1 < P.bh && gx + 1 < P.bw;
    const int s00 = iy * kMetricsHaloX + ix, s01 = s00 + 1, s10 = s00 + kMetricsHaloX, s11 = s10 + 1;
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        double t = 0.0;
        if (window) {
            const unsigned w1 = sS1[c][s00] + sS1[c][s01] + sS1[c][s10] + sS1[c][s11];
            const unsigned w2 = sS2[c][s00] + sS2[c][s01] + sS2[c][s10] + sS2[c][s11];
            const M wss = sSS[c][s00] + sSS[c][s01] + sSS[c][s10] + sSS[c][s11];
            const M w12 = sS12[c][s00] + sS12[c][s01] + sS12[c][s10] + sS12[c][s11];
            t = metrics_window_t(static_cast<double>(w1), static_cast<double>(w2), static_cast<double>(wss), static_cast<double>(w12), P.c1, P.c2);
        }
        unsigned long long e = sse[c];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { // a fixed tree: the same order on every run
            t += __shfl_down(t, d, 64);
            e += __shfl_down(e, d, 64);
        }
        if (lane == 0) sWaveT[c][wave] = t, sWaveE[c][wave] = e;
    }
    __syncthreads();
    if (tid < C) {
        double t = sWaveT[tid][0];
        unsigned long long e = sWaveE[tid][0];
#pragma unroll
        for (int w = 1; w < kMetricsThreads / 64; ++w) t += sWaveT[tid][w], e += sWaveE[tid][w];
        MetricsPartial r;
        r.ssimSum = t;
        r.sse = e;
        part[(static_cast<size_t>(n) * C + tid) * tiles + tile] = r;
    }
}

// one block per (image, channel): thread i adds partials i, i + 256, ... in index order, then a fixed tree over the threads
__global__ __launch_bounds__(kMetricsFoldThreads) void frame_metrics_fold_kernel(const MetricsPartial* __restrict__ part, int tiles, unsigned long long pixels,
                                                                                unsigned long long windows, double maxval,
                                                                                snnhip_frame_metrics_row* __restrict__ rows, float* __restrict__ out) {
    __shared__ double sT[kMetricsFoldThreads];
    __shared__ unsigned long long sE[kMetricsFoldThreads];
    const int tid = threadIdx.x;
    const MetricsPartial* p = part + static_cast<size_t>(blockIdx.x) * tiles;
    double t = 0.0;
    unsigned long long e = 0ull;
    for (int i = tid; i < tiles; i += kMetricsFoldThreads) t += p[i].ssimSum, e += p[i].sse;
    sT[tid] = t, sE[tid] = e;
    for (int d = kMetricsFoldThreads / 2; d > 0; d >>= 1) {
        __syncthreads();
        if (tid < d) sT[tid] += sT[tid + d], sE[tid] += sE[tid + d];
    }
    if (tid == 0) {
        snnhip_frame_metrics_row r;
        r.sse = sE[0];
        r.pixels = pixels;
        r.windows = windows;
        r.ssim_sum = sT[0];
        rows[blockIdx.x] = r;
        const double psnr = r.sse == 0ull ? static_cast<double>(INFINITY) : 10.0 * log10(maxval * maxval * static_cast<double>(pixels) / static_cast<double>(r.sse));
        out[2 * blockIdx.x] = static_cast<float>(psnr);
        out[2 * blockIdx.x + 1] = static_cast<float>(r.ssim_sum / static_cast<double>(windows));
    }
}

struct FrameMetricsPlan : snnhip_plan {
    snnhip_frame_metrics_desc d;
    MetricsParams P;
    MetricsPartial* part = nullptr;
    snnhip_frame_metrics_row* rows = nullptr;

    template <typename T, int C>
    void launch(const snnhip_tensor* a, const snnhip_tensor* b) {
        const dim3 grid(static_cast<unsigned>(P.N) * static_cast<unsigned>(P.tilesX) * static_cast<unsigned>(P.tilesY));
        SNNHIP_LAUNCH((frame_metrics_tile_kernel<T, C>), grid, dim3(kMetricsThreads), 0, ctx->stream, P, reinterpret_cast<const T*>(a->data),
                      reinterpret_cast<const T*>(b->data), part);
    }
    template <typename T>
    void launch_c(const snnhip_tensor* a, const snnhip_tensor* b) {
        switch (d.C) {
        case 1: launch<T, 1>(a, b); break;
        case 2: launch<T, 2>(a, b); break;
        case 3: launch<T, 3>(a, b); break;
        default: launch<T, 4>(a, b); break;
        }
    }

    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        SNNHIP_REQUIRE(nIn == 2, "frame_metrics: expects 2 inputs (the test frame and the reference frame), got %d", nIn);
        for (int i = 0; i < 2; ++i) {
            SNNHIP_REQUIRE(in[i]->dtype == d.dtype, "frame_metrics: input %d has dtype %d, the plan was built for %d", i, in[i]->dtype, d.dtype);
            SNNHIP_REQUIRE(dims_match(in[i], d.N, d.H, d.W, d.C), "frame_metrics: input %d is %dx%dx%dx%d, the plan was built for %dx%dx%dx%d", i, in[i]->n, in[i]->h,
                           in[i]->w, in[i]->c, d.N, d.H, d.W, d.C);
        }
        SNNHIP_REQUIRE(out->dtype == SNNHIP_F32 && dims_match(out, d.N, 1, d.C, 2),
                       "frame_metrics: the output is %dx%dx%dx%d of dtype %d, expected fp32 %dx1x%dx2 ({psnr_db, ssim} per image and channel)", out->n, out->h, out->w,
                       out->c, out->dtype, d.N, d.C);
        if (d.dtype == SNNHIP_U8) launch_c<unsigned char>(in[0], in[1]);
        else launch_c<unsigned short>(in[0], in[1]);
        SNNHIP_CHECK_HIP(hipGetLastError());
        const unsigned long long pixels = static_cast<unsigned long long>(d.H) * d.W;
        const unsigned long long windows = static_cast<unsigned long long>(P.bh - 1) * (P.bw - 1);
        SNNHIP_LAUNCH(frame_metrics_fold_kernel, dim3(static_cast<unsigned>(d.N * d.C)), dim3(kMetricsFoldThreads), 0, ctx->stream, part, P.tilesX * P.tilesY, pixels,
                      windows, static_cast<double>(d.maxval), rows, out->data);
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }
};

} // namespace
} // namespace snnhip

using namespace snnhip;

extern "C" {

double snnhip_frame_metrics_psnr(unsigned long long sse, unsigned long long pixels, int maxval) {
    if (sse == 0ull) return static_cast<double>(INFINITY);
    const double m = static_cast<double>(maxval);
    return 10.0 * std::log10(m * m * static_cast<double>(pixels) / static_cast<double>(sse));
}

int snnhip_frame_metrics_plan_create(snnhip_ctx* ctx, const snnhip_frame_metrics_desc* desc, snnhip_plan** out) {
    SNNHIP_REQUIRE(ctx && desc && out, "frame_metrics_plan_create: null argument");
    SNNHIP_REQUIRE(desc->N > 0, "frame_metrics desc: bad batch %d", desc->N);
    SNNHIP_REQUIRE(desc->C >= 1 && desc->C <= 4, "frame_metrics desc: %d channels (1..4, interleaved)", desc->C);
    SNNHIP_REQUIRE(desc->dtype == SNNHIP_U8 || desc->dtype == SNNHIP_U16, "frame_metrics desc: dtype %d (SNNHIP_U8 or SNNHIP_U16)", desc->dtype);
    SNNHIP_REQUIRE(desc->H >= 8 && desc->W >= 8, "frame_metrics desc: %dx%d is smaller than one 8x8 window", desc->H, desc->W);
    const int bits = desc->dtype == SNNHIP_U8 ? 8 : 16;
    SNNHIP_REQUIRE(desc->shift >= 0 && desc->shift < bits && (bits == 16 || desc->shift == 0), "frame_metrics desc: shift %d (0 for 8-bit frames, 0..15 for 16-bit containers)",
                   desc->shift);
    SNNHIP_REQUIRE(desc->maxval >= 1, "frame_metrics desc: maxval %d (at least 1)", desc->maxval);
    SNNHIP_REQUIRE((static_cast<long long>(desc->maxval) << desc->shift) < (1ll << bits), "frame_metrics desc: maxval %d << shift %d does not fit %d bits", desc->maxval,
                   desc->shift, bits);
    const int tilesX = up_div(desc->W, kMetricsTileW), tilesY = up_div(desc->H, kMetricsTileH);
    const double blocks = static_cast<double>(desc->N) * tilesX * tilesY;
    const double elems = static_cast<double>(desc->N) * desc->H * desc->W * desc->C;
    SNNHIP_REQUIRE(blocks * desc->C < 2147483648.0 && elems < 9.0e15, "frame_metrics desc: %dx%dx%dx%d is too large", desc->N, desc->H, desc->W, desc->C);

    auto* plan = new FrameMetricsPlan();
    plan->ctx = ctx;
    plan->numInputs = 2;
    plan->dtype = desc->dtype;
    plan->anyDtype = true; // two raw frames in, an fp32 tensor out: run() checks all three itself
    plan->rawInput = desc->dtype;
    plan->d = *desc;
    plan->P = MetricsParams{};
    plan->P.N = desc->N;
    plan->P.H = desc->H;
    plan->P.W = desc->W;
    plan->P.bh = desc->H >> 2;
    plan->P.bw = desc->W >> 2;
    plan->P.tilesX = tilesX;
    plan->P.tilesY = tilesY;
    plan->P.shift = desc->shift;
    const double m = static_cast<double>(desc->maxval);
    plan->P.c1 = 0.01 * 0.01 * m * m * 64.0;        // left to right, as tests/metrics_ref.py evaluates it
    plan->P.c2 = 0.03 * 0.03 * m * m * 64.0 * 63.0;
    const size_t nPart = static_cast<size_t>(desc->N) * desc->C * tilesX * tilesY, nRows = static_cast<size_t>(desc->N) * desc->C;
    if (dev_malloc(&plan->part, nPart * sizeof(MetricsPartial), "frame_metrics partials") != hipSuccess) {
        delete plan;
        set_error("frame_metrics_plan_create: out of device memory for %zu partials", nPart);
        return SNNHIP_E_NOMEM;
    }
    plan->deviceAllocs.push_back(plan->part);
    if (dev_malloc(&plan->rows, nRows * sizeof(snnhip_frame_metrics_row), "frame_metrics rows") != hipSuccess) {
        delete plan;
        set_error("frame_metrics_plan_create: out of device memory for %zu rows", nRows);
        return SNNHIP_E_NOMEM;
    }
    plan->deviceAllocs.push_back(plan->rows);
    plan->inDims[0] = plan->outDims[0] = desc->N;
    plan->inDims[1] = desc->H;
    plan->inDims[2] = desc->W;
    plan->inDims[3] = desc->C;
    plan->outDims[1] = 1;
    plan->outDims[2] = desc->C;
    plan->outDims[3] = 2;
    plan->bytes = 2.0 * elems * (bits / 8) + 2.0 * static_cast<double>(nPart) * sizeof(MetricsPartial); // both frames once, the partials written and read
    plan->flops = elems * 8.0; // per sample: two sums, three products and their adds
    char buf[256];
    snprintf(buf, sizeof(buf), "frame_metrics_u%d c=%d tile=%dx%d %dx%dx%d maxval=%d shift=%d windows=%dx%d partials=%d kernel=frame_metrics_tile_kernel+frame_metrics_fold_kernel",
             bits, desc->C, kMetricsTileH, kMetricsTileW, desc->N, desc->H, desc->W, desc->maxval, desc->shift, plan->P.bh - 1, plan->P.bw - 1, tilesX * tilesY);
    plan->desc = buf;
    *out = plan;
    return SNNHIP_OK;
}

int snnhip_frame_metrics_read(snnhip_plan* plan, snnhip_frame_metrics_row* rows, int max_rows) {
    SNNHIP_REQUIRE(plan && rows, "frame_metrics_read: null argument");
    auto* p = dynamic_cast<FrameMetricsPlan*>(plan);
    SNNHIP_REQUIRE(p, "frame_metrics_read: not a frame_metrics plan (%s)", plan->desc.c_str());
    const int n = p->d.N * p->d.C;
    SNNHIP_REQUIRE(max_rows >= n, "frame_metrics_read: room for %d rows, the plan writes %d (N * C)", max_rows, n);
    SNNHIP_CHECK_HIP(hipStreamSynchronize(p->ctx->stream));
    SNNHIP_CHECK_HIP(hipMemcpy(rows, p->rows, static_cast<size_t>(n) * sizeof(snnhip_frame_metrics_row), hipMemcpyDeviceToHost));
    return n;
}

} // extern "C"
