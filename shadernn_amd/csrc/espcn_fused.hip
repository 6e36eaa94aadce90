// espcn_fused.hip -- the fp32 kernels of the ESPCN-shaped part of the hot path (BASELINE config 2), their launch functions and their host-side weight
// images (espcn_fused.h).  The rules that select them are in the chain planner, chain_fuse.hip.
//
// The reference runs one compute dispatch + one full barrier per layer (core/src/ic2/vulkanRenderpass.cpp:257-259)
// and round-trips every intermediate through a texture.  Here a linear chain of plans is rewritten into two kernels:
//
//   kernel A  conv KxK (IC=1 -> 16, K in {3,5}) + act  ->  conv 3x3 (16 -> 16) + act       [fp32 MFMA, LDS-resident mid tensor]
//             replaces two passes of shadertemplate_vk_conv2d.comp:148-347
//   kernel B  conv 3x3 (16 -> 4) + act  ->  depth-to-space(2) + tanh                         [VALU, HBM-bound]
//             replaces shadertemplate_vk_conv2d.comp + shadertemplate_vk_subpixel.comp:43-71
//
// Kernel A, per 64x8 output tile (256 threads = 4 waves, 46 KB LDS, 3 blocks/CU = __launch_bounds__(256, 3)):
//   phase 0  input halo tile (70x14, 1 channel) -> LDS, zero outside the image (constant padding)
//   phase 1  conv1 on the 66x10 halo region as a GEMM  D[oc][px] = W1[oc][tap] * im2col[tap][px]  with
//            v_mfma_f32_16x16x4_f32 (K = 25 taps padded to 28), bias/BN/act fused, zeroed outside the image (it is
//            conv2's zero padding), written to LDS as [row][col][16ch] with a 16-byte-slot XOR swizzle
//   phase 2  conv2 as 9 taps x 4 MFMAs per 16-pixel group: B operand = one ds_read_b128 (4 input channels of one
//            pixel), A operand = weights held in 36 VGPRs for the whole kernel; 8 groups (=accumulators) per wave
//   epilogue bias/BN/act, 16-byte stores: one wave store = 16 pixels x 64 B contiguous NHWC
// fp32 MFMA is bit-for-bit an fp32 fma chain (no reduced precision), so the 1e-4 parity bound holds as for VALU code.
#include <hip/hip_ext.h>

#include "espcn_d2s_mfma.h"
#include "espcn_fused.h"
#include "snnhip_internal.h"

// developer hook: tools/tune_espcn.hip defines SNNHIP_STAMP(k) to record s_memtime per wave and phase
#ifndef SNNHIP_STAMP
#define SNNHIP_STAMP(k)
#endif

namespace snnhip {

// input-resolution pixels per block (declared for the chain planner in espcn_fused.h)
constexpr int A_TW = 64, A_TH = 8;
constexpr int W_TH = 16, W_WPS = 2; // Winograd kernel A: tile 32 x W_TH, W_WPS blocks (waves/SIMD) per CU
struct WinoTile {
    static constexpr int TW = 32;
};
constexpr int W_TW = WinoTile::TW;
constexpr int B_TW = 32, B_TH = 8;
constexpr int BR_TW = kD2sMfmaTW, BR_TH = kD2sMfmaTH; // rule B for upscale 3 / 4 (espcn_d2s_mfma.hip)
constexpr int BW_TW = 64, BW_TH = 16; // Winograd kernel B: its tile is local to the kernel, checked against this pair there

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// K1 = first conv's kernel size (3 or 5), pad = K1/2.  TW multiple of 16, TH multiple of 4.
template <int K1, int TW, int TH, bool SIMPLE, int U = 3, int WPS = 3>
__global__ __launch_bounds__(256, WPS) void conv_kxk_c1o16_conv3x3_c16o16_kernel(FusedAParams p, const float* __restrict__ x,
                                                                            const float* __restrict__ wA1, const float* __restrict__ wA2,
                                                                            const float* __restrict__ ep1, const float* __restrict__ ep2,
                                                                            float* __restrict__ y) {
    constexpr int P1 = K1 / 2;
    constexpr int C1W = TW + 2, C1H = TH + 2;                 // conv1 output region needed by conv2 (halo 1)
    constexpr int INW = TW + 2 + 2 * P1, INH = TH + 2 + 2 * P1; // input region needed by conv1 on that region
    constexpr int KS1 = (K1 * K1 + 3) / 4;                    // MFMA K-steps of conv1
    constexpr int NG1 = (C1H * C1W + 15) / 16;                // 16-pixel groups of phase 1
    constexpr int GPR = TW / 16;                              // groups per output row
    constexpr int RPW = TH / 4;                               // output rows per wave
    constexpr int G = GPR * RPW;                              // groups (= accumulators) per wave in phase 2

    __shared__ __attribute__((aligned(16))) float smem[C1H * C1W * 16 + INH * INW];
    float* s_c1 = smem;
    float* s_in = smem + C1H * C1W * 16;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int px = lane & 15, g = lane >> 4;

    int b = xcd_tile_order(blockIdx.x, gridDim.x);
    const int tx = b % p.tilesX;
    b /= p.tilesX;
    const int ty = b % p.tilesY;
    const int n = b / p.tilesY;
    const int x0 = tx * TW, y0 = ty * TH;
    const float* xn = x + static_cast<size_t>(n) * p.H * p.W;

    SNNHIP_STAMP(0);
    // ---- phase 0: input tile (origin y0-1-P1, x0-1-P1), zero padded
    {
        constexpr int NLD = (INH * INW + 255) / 256;
        float v[NLD];
#pragma unroll
        for (int k = 0; k < NLD; ++k) { // all loads in flight before the first use
            const int idx = tid + k * 256;
            const int r = idx / INW, c = idx - r * INW;
            const int gy = y0 - 1 - P1 + r, gx = x0 - 1 - P1 + c;
            v[k] = 0.0f;
            if (idx < INH * INW && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) v[k] = xn[static_cast<size_t>(gy) * p.W + gx];
        }
#pragma unroll
        for (int k = 0; k < NLD; ++k)
            if (tid + k * 256 < INH * INW) s_in[tid + k * 256] = v[k];
    }

    // ---- weights -> registers (host packed them in lane order)
    float a1[KS1];
#pragma unroll
    for (int s = 0; s < KS1; ++s) a1[s] = wA1[s * 64 + lane];
    float a2[36];
#pragma unroll
    for (int t = 0; t < 36; ++t) a2[t] = wA2[t * 64 + lane];
    float sc1[4], sh1[4], sc2[4], sh2[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sc1[r] = ep1[(4 * g + r) * 2];
        sh1[r] = ep1[(4 * g + r) * 2 + 1];
        sc2[r] = ep2[(4 * g + r) * 2];
        sh2[r] = ep2[(4 * g + r) * 2 + 1];
    }
    // this lane's tap offsets for conv1: K-step s covers taps 4s..4s+3, lane group g supplies tap 4s+g
    int off1[KS1];
    bool tapok[KS1];
#pragma unroll
    for (int s = 0; s < KS1; ++s) {
        int t = 4 * s + g;
        tapok[s] = t < K1 * K1;
        if (!tapok[s]) t = K1 * K1 - 1;
        off1[s] = (t / K1) * INW + (t % K1);
    }
    SNNHIP_STAMP(1);
    __syncthreads();
    SNNHIP_STAMP(2);

    // ---- phase 1: conv1 over the C1H x C1W halo region, pixels flattened into 16-wide groups.
    // U groups per iteration = U independent MFMA accumulation chains (one chain alone is bound by the 40-cycle
    // dependent-accumulator latency of v_mfma_f32_16x16x4_f32).
    for (int grp0 = wv * U; grp0 < NG1; grp0 += 4 * U) {
        f32x4 acc[U];
        const float* src[U];
        int rr[U], cc[U];
        bool valid[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int pi = (grp0 + u) * 16 + px;
            valid[u] = pi < C1H * C1W;
            const int pc = valid[u] ? pi : C1H * C1W - 1;
            rr[u] = pc / C1W;
            cc[u] = pc - rr[u] * C1W;
            src[u] = s_in + rr[u] * INW + cc[u];
            acc[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int s = 0; s < KS1; ++s) {
            float bv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                bv[u] = src[u][off1[s]];
                if (!tapok[s]) bv[u] = 0.0f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[s], bv[u], acc[u], 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int gy = y0 - 1 + rr[u], gx = x0 - 1 + cc[u];
            const bool inside = gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
            float4 o;
            o.x = inside ? apply_act<SIMPLE>(p.act1, fmaf(acc[u][0], sc1[0], sh1[0]), 0.0f) : 0.0f;
            o.y = inside ? apply_act<SIMPLE>(p.act1, fmaf(acc[u][1], sc1[1], sh1[1]), 0.0f) : 0.0f;
            o.z = inside ? apply_act<SIMPLE>(p.act1, fmaf(acc[u][2], sc1[2], sh1[2]), 0.0f) : 0.0f;
            o.w = inside ? apply_act<SIMPLE>(p.act1, fmaf(acc[u][3], sc1[3], sh1[3]), 0.0f) : 0.0f;
            if (valid[u]) {
                const int slot = g ^ (((cc[u] >> 2) & 1) << 1); // conflict-free ds_read_b128 in phase 2 for every tap shift
                *reinterpret_cast<float4*>(s_c1 + (rr[u] * C1W + cc[u]) * 16 + slot * 4) = o;
            }
        }
    }
    SNNHIP_STAMP(3);
    __syncthreads();
    SNNHIP_STAMP(4);

    // ---- phase 2: conv2, G accumulators per wave
    f32x4 acc2[G];
#pragma unroll
    for (int gi = 0; gi < G; ++gi) acc2[gi] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int fy = tap / 3, fx = tap % 3;
        float4 bv[G];
#pragma unroll
        for (int gi = 0; gi < G; ++gi) {
            const int row = wv * RPW + gi / GPR, col0 = (gi % GPR) * 16;
            const int cc = col0 + px + fx;
            const int slot = g ^ (((cc >> 2) & 1) << 1);
            bv[gi] = *reinterpret_cast<const float4*>(s_c1 + ((row + fy) * C1W + cc) * 16 + slot * 4);
        }
#pragma unroll
        for (int gi = 0; gi < G; ++gi) acc2[gi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[tap * 4 + 0], bv[gi].x, acc2[gi], 0, 0, 0);
#pragma unroll
        for (int gi = 0; gi < G; ++gi) acc2[gi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[tap * 4 + 1], bv[gi].y, acc2[gi], 0, 0, 0);
#pragma unroll
        for (int gi = 0; gi < G; ++gi) acc2[gi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[tap * 4 + 2], bv[gi].z, acc2[gi], 0, 0, 0);
#pragma unroll
        for (int gi = 0; gi < G; ++gi) acc2[gi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[tap * 4 + 3], bv[gi].w, acc2[gi], 0, 0, 0);
    }

    SNNHIP_STAMP(5);
    // ---- epilogue: lane holds output channels 4g..4g+3 of pixel (row, col0+px)
    float* yn = y + static_cast<size_t>(n) * p.H * p.W * 16;
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
        const int gy = y0 + wv * RPW + gi / GPR, gx = x0 + (gi % GPR) * 16 + px;
        if (gy < p.H && gx < p.W) {
            float4 o;
            o.x = apply_act<SIMPLE>(p.act2, fmaf(acc2[gi][0], sc2[0], sh2[0]), 0.0f);
            o.y = apply_act<SIMPLE>(p.act2, fmaf(acc2[gi][1], sc2[1], sh2[1]), 0.0f);
            o.z = apply_act<SIMPLE>(p.act2, fmaf(acc2[gi][2], sc2[2], sh2[2]), 0.0f);
            o.w = apply_act<SIMPLE>(p.act2, fmaf(acc2[gi][3], sc2[3], sh2[3]), 0.0f);
            *reinterpret_cast<float4*>(yn + (static_cast<size_t>(gy) * p.W + gx) * 16 + g * 4) = o;
        }
    }
    SNNHIP_STAMP(6);
}

// Kernel A, Winograd variant (default): same fusion, but conv2 (3x3, 16 -> 16) is evaluated as F(2x2, 3x3):
//     Y = At [ (G g Gt) .* (Bt d B) ] A      per 2x2 output block and (oc, ic) pair            (Lavin & Gray 2016)
// which needs 16 multiplies per 4 outputs instead of 36 -> 2.25x fewer MFMA flops for the layer that owns 70 % of the
// network's arithmetic.  All transform coefficients are 0, +-1 (input/output) or +-1/2 (weights, done on the host in
// double precision), so the fp32 result differs from the direct sum by a few ulp (parity tests: <= 1e-4 as before).
//   block   = 32x16 output pixels = 16x8 Winograd tiles; 256 threads = 4 waves; 58.6 KB LDS -> 2 blocks/CU
//   phase 1 = conv1 (MFMA, as in the direct kernel) into LDS [row][col parity][col/2][16ch]; the column de-interleave makes
//             the stride-2 tile reads of phase 2 consecutive, the slot XOR (bit 2 of the linear pixel index) makes them
//             conflict-free for the ds_read_b128 lane groups
//   phase 2 = per wave 2 groups of 16 tiles (one tile row each): lane (tile t = lane%16, g = lane/16) loads its 4x4 input
//             patch for channels 4g..4g+3 (16 ds_read_b128), then per transform column nu: input transform (VALU, float4
//             adds), 16 MFMAs  M[xi][oc][tile] += U[xi,nu][oc][ic] * V[xi,nu][ic][tile]  (v_mfma_f32_16x16x4_f32, U read
//             from LDS as one b128 per position), output transform folded into the 2x2x4 result registers
//   epilogue= bias/BN/act, four 16-byte stores per lane
// (the conv1 K-step -> tap assignment, wino_conv1_tap: espcn_fused.h)
// AM: 0 = any activation (run-time switch), 1 = cheap family (branch-free med3 form), 2 = both layers ReLU
template <int AM>
__device__ __forceinline__ float act_mode(const ActCfg& a, float v) {
    if (AM == 2) return fmaxf(v, 0.0f);
    if (AM == 1) return apply_act<true>(a, v, 0.0f);
    return epi_act(a.act, a.leaky, v, 0.0f);
}

// rule A's kernel (fp32 input) and rule A8's (8-bit input): one body, espcn_wino_a_body.h
template <int K1, int TH, int AM, int WPS>
__global__ __launch_bounds__(256, WPS) void conv_kxk_c1o16_wino3x3_c16o16_kernel(FusedAParams p, const float* __restrict__ x,
                                                                           const float* __restrict__ wA1, const float* __restrict__ wU,
                                                                           const float* __restrict__ ep1, const float* __restrict__ ep2,
                                                                           float* __restrict__ y) {
    typedef float TIn;
    constexpr U8InCfg qin{0.0f, 0.0f};
    constexpr U16InCfg qin16{0.0f, 0.0f, 0};
#include "espcn_wino_a_body.h"
}

template <int K1, int TH, int AM, int WPS>
__global__ __launch_bounds__(256, WPS) void conv_kxk_c1o16_wino3x3_c16o16_u8_kernel(FusedAParams p, U8InCfg qin, const unsigned char* __restrict__ x,
                                                                              const float* __restrict__ wA1, const float* __restrict__ wU,
                                                                              const float* __restrict__ ep1, const float* __restrict__ ep2,
                                                                              float* __restrict__ y) {
    typedef unsigned char TIn;
    constexpr U16InCfg qin16{0.0f, 0.0f, 0};
#include "espcn_wino_a_body.h"
}

// the 16-bit form (snnhip_u16_in_plan_create folded in): its own parameter block, the 8-bit kernel's stays what it is
template <int K1, int TH, int AM, int WPS>
__global__ __launch_bounds__(256, WPS) void conv_kxk_c1o16_wino3x3_c16o16_u16_kernel(FusedAParams p, U16InCfg qin16, const unsigned short* __restrict__ x,
                                                                               const float* __restrict__ wA1, const float* __restrict__ wU,
                                                                               const float* __restrict__ ep1, const float* __restrict__ ep2,
                                                                               float* __restrict__ y) {
    typedef unsigned short TIn;
    constexpr U8InCfg qin{0.0f, 0.0f};
#include "espcn_wino_a_body.h"
}

// conv 3x3 (16 -> 4, zero padding 1) + act, then depth-to-space(2) + tanh.  One thread = one input-resolution pixel
// = a 2x2 block of the output image.  LDS tile [TH+2][TW+2] pixels, 64 B each, 16-byte slots XOR-swizzled (conflict-free
// b128 reads for 64 consecutive pixels, 21.8 KB per block -> 7 blocks/CU); weights are wave-uniform => scalar loads, FMAs take them as SGPR operands.
// rule B's kernel (fp32 output) and rule B8's (8-bit output): one body, espcn_d2s_b_body.h
template <int TW, int TH, bool SIMPLE>
__global__ __launch_bounds__(256) void conv3x3_c16o4_d2s_tanh_kernel(FusedBParams p, const float* __restrict__ x, const float* __restrict__ w,
                                                                     const float* __restrict__ ep, float* __restrict__ y) {
    typedef float TOut;
    constexpr U8OutCfg qout{0.0f, 0.0f};
    constexpr U16OutCfg qout16{0.0f, 0.0f, 0.0f, 0};
#include "espcn_d2s_b_body.h"
}

template <int TW, int TH, bool SIMPLE>
__global__ __launch_bounds__(256) void conv3x3_c16o4_d2s_tanh_u8_kernel(FusedBParams p, U8OutCfg qout, const float* __restrict__ x, const float* __restrict__ w,
                                                                        const float* __restrict__ ep, unsigned char* __restrict__ y) {
    typedef unsigned char TOut;
    constexpr U16OutCfg qout16{0.0f, 0.0f, 0.0f, 0};
#include "espcn_d2s_b_body.h"
}

// the 16-bit form (snnhip_u16_out_plan_create folded in)
template <int TW, int TH, bool SIMPLE>
__global__ __launch_bounds__(256) void conv3x3_c16o4_d2s_tanh_u16_kernel(FusedBParams p, U16OutCfg qout16, const float* __restrict__ x, const float* __restrict__ w,
                                                                         const float* __restrict__ ep, unsigned short* __restrict__ y) {
    typedef unsigned short TOut;
    constexpr U8OutCfg qout{0.0f, 0.0f};
#include "espcn_d2s_b_body.h"
}

// Kernel B, Winograd variant (default): conv 3x3 (16 -> 4) as F(2x2, 3x3) on the matrix cores, then depth-to-space(2) + tanh.
// With only 4 output channels a 16-wide MFMA tile would be 3/4 padding; v_mfma_f32_4x4x1_16B_f32 instead runs 16
// independent 4x4x1 outer products per instruction: block = 4 Winograd tiles, rows = the 4 output channels, one input
// channel per instruction.  Lane l is Winograd tile l of its wave (64 tiles = 32 x 2), so both transforms are lane-local:
//   per channel quad q: 16 ds_read_b128 (the tile's 4x4 input patch), Bt d B (32 float4 adds), then per transform
//   position 4 MFMAs  M[pos][oc][tile] += U[pos][oc][ic] * V[pos][ic][tile]   (U: one broadcast ds_read_b128 per position)
//   after the 4 quads: At M A (24 float4 adds), bias/BN/act, tanh, and the 4x4 block of output pixels the tile maps to
//   under depth-to-space is written as four 16-byte stores.
// 256 MFMAs (8 cycles each) + ~800 VALU per 256 pixels instead of 9216 scalar FMAs.  fp32 MFMA executes on the same FMA
// lanes as VALU code (tools/ubench_issue.hip: their issue times add up), so the win is the 2.25x cut in multiplies plus the
// removal of the per-tap scalar weight loads.  Block = 64 x 16 pixels, 80 KB LDS -> 2 blocks/CU.
template <bool SIMPLE>
__global__ __launch_bounds__(256, 2) void conv3x3_c16o4_wino_d2s_tanh_kernel(FusedBParams p, const float* __restrict__ x, const float* __restrict__ wU,
                                                                        const float* __restrict__ ep, float* __restrict__ y) {
    constexpr int TW = 64, TH = 16, XW = TW + 2, XH = TH + 2, HALF = XW / 2;
    static_assert(TW == BW_TW && TH == BW_TH, "the planner sizes this kernel's grid with BW_TW x BW_TH");
    constexpr int NPIX = XH * XW, NLD = (NPIX + 255) / 256; // halo pixels per tile; float4 per thread and channel quad
    __shared__ __attribute__((aligned(16))) float s_x[NPIX * 16];
    __shared__ __attribute__((aligned(16))) float s_U[1024];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ntiles = p.tilesX * p.tilesY * p.N;

    // Persistent blocks (grid = 2 per CU) with a quad-granular software pipeline: the tile is consumed one channel quad
    // (16-byte slot of every pixel) at a time, so as soon as all waves are done with quad q of this tile, quad q of the NEXT
    // tile -- fetched into 5 float4 registers per thread while quad q was being computed -- overwrites it.  The HBM/MALL stream
    // and the MFMA/VALU work overlap inside every block; without this all blocks of a launch load together and compute
    // together (measured: 44 % of the block lifetime in the load phase).
    // Halo tile layout: pixel (r, c) at linear index pl = r*XW + (c&1)*HALF + (c>>1) (columns de-interleaved so that the
    // stride-2 patch reads of 32 adjacent tiles are consecutive), 16-byte slot q ^ ((pl>>2)&3) (conflict-free ds_read_b128).
    auto tile_origin = [&](int t, int& n, int& x0, int& y0) {
        int b = xcd_tile_order(t, ntiles);
        const int tx = b % p.tilesX;
        b /= p.tilesX;
        const int ty = b % p.tilesY;
        n = b / p.tilesY;
        x0 = tx * TW;
        y0 = ty * TH;
    };
    // tile-independent staging descriptors of this thread's halo pixels
    int rc[NLD], ldst[NLD]; // (r << 8) | c   and   byte offset of slot bits 0 of the pixel, swizzle term folded in
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
        const int pix = tid + k * 256;
        const int pp = pix < NPIX ? pix : 0;
        const int r = pp / XW, c = pp - r * XW;
        const int pl = r * XW + (c & 1) * HALF + (c >> 1);
        rc[k] = pix < NPIX ? ((r << 8) | c) : -1;
        ldst[k] = pl * 64 + (((pl >> 2) & 3) << 4);
    }
    float4 v[NLD];
    const float* xt = nullptr; // image base of the tile being fetched
    int fx0 = 0, fy0 = 0;
    auto begin_fetch = [&](int t) {
        int n;
        tile_origin(t, n, fx0, fy0);
        xt = x + static_cast<size_t>(n) * p.H * p.W * 16;
    };
    auto issue_loads = [&](int q) {
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int gy = fy0 - 1 + (rc[k] >> 8), gx = fx0 - 1 + (rc[k] & 255);
            v[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (rc[k] >= 0 && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W)
                v[k] = *reinterpret_cast<const float4*>(xt + (static_cast<size_t>(gy) * p.W + gx) * 16 + q * 4);
        }
    };
    auto store_lds = [&](int q) {
#pragma unroll
        for (int k = 0; k < NLD; ++k)
            if (rc[k] >= 0) *reinterpret_cast<float4*>(reinterpret_cast<char*>(s_x) + (ldst[k] ^ (q << 4))) = v[k];
    };

    int tile = blockIdx.x;
    if (tile >= ntiles) return;
    SNNHIP_STAMP(0);
    begin_fetch(tile);
    reinterpret_cast<float4*>(s_U)[tid] = reinterpret_cast<const float4*>(wU)[tid];
    { // first tile: all four quads in flight at once
        float4 v0[4][NLD];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            issue_loads(q);
#pragma unroll
            for (int k = 0; k < NLD; ++k) v0[q][k] = v[k];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int k = 0; k < NLD; ++k) v[k] = v0[q][k];
            store_lds(q);
        }
    }
    SNNHIP_STAMP(1);
    __syncthreads();
    SNNHIP_STAMP(2);

    float sc[4], sh[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        sc[k] = ep[2 * k];
        sh[k] = ep[2 * k + 1];
    }
    const int tcol = lane & 31, trow = 2 * wv + (lane >> 5); // this lane's Winograd tile: output pixels (2 trow + a, 2 tcol + b)
    int off[4][4];                                             // byte offset of patch pixel (i, j), slot bits of quad 0
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int pl = (2 * trow + i) * XW + (j & 1) * HALF + tcol + (j >> 1);
            off[i][j] = pl * 64 + (((pl >> 2) & 3) << 4);
        }
    const char* sxb = reinterpret_cast<const char*>(s_x);
    const float* uLane = s_U + (lane & 3) * 4; // + (pos*4 + q)*16 floats: U[pos][oc = lane&3][ic = 4q .. 4q+3]

    for (;;) {
        int n, x0, y0;
        tile_origin(tile, n, x0, y0);
        const int next = tile + gridDim.x;
        const bool more = next < ntiles;
        if (more) begin_fetch(next);

        f32x4 M[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (more) issue_loads(q);
            f32x4 d[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) d[i][j] = *reinterpret_cast<const f32x4*>(sxb + (off[i][j] ^ (q << 4)));
                // V = Bt d B, in place: columns first (d B), then rows
#ifndef SNNHIP_BW_SKIP_TRANSFORM
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 e0 = d[i][0] - d[i][2], e1 = d[i][1] + d[i][2], e2 = d[i][2] - d[i][1], e3 = d[i][1] - d[i][3];
                d[i][0] = e0;
                d[i][1] = e1;
                d[i][2] = e2;
                d[i][3] = e3;
            }
#pragma unroll
            for (int nu = 0; nu < 4; ++nu) {
                const f32x4 v0 = d[0][nu] - d[2][nu], v1 = d[1][nu] + d[2][nu], v2 = d[2][nu] - d[1][nu], v3 = d[1][nu] - d[3][nu];
                d[0][nu] = v0;
                d[1][nu] = v1;
                d[2][nu] = v2;
                d[3][nu] = v3;
            }
#endif
            // 16 positions x 4 channels; 4 positions in flight so consecutive MFMAs never share an accumulator
#pragma unroll
            for (int xi = 0; xi < 4; ++xi) {
                f32x4 u4[4];
#pragma unroll
                for (int nu = 0; nu < 4; ++nu) u4[nu] = *reinterpret_cast<const f32x4*>(uLane + ((xi * 4 + nu) * 4 + q) * 16);
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int nu = 0; nu < 4; ++nu) {
                        const int pos = xi * 4 + nu;
                        if (q == 0 && k == 0)
                            M[pos] = __builtin_amdgcn_mfma_f32_4x4x1f32(u4[nu][k], d[xi][nu][k], f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
                        else
                            M[pos] = __builtin_amdgcn_mfma_f32_4x4x1f32(u4[nu][k], d[xi][nu][k], M[pos], 0, 0, 0);
                    }
            }
            if (more) {
                __syncthreads(); // every wave has consumed quad q of this tile
                store_lds(q);
            }
        }
        SNNHIP_STAMP(3);

        // ---- Y = At M A  (per output channel = accumulator register)
        f32x4 Y[2][2];
        {
            f32x4 T[2][4];
#pragma unroll
            for (int nu = 0; nu < 4; ++nu) {
                T[0][nu] = M[0 * 4 + nu] + M[1 * 4 + nu] + M[2 * 4 + nu];
                T[1][nu] = M[1 * 4 + nu] - M[2 * 4 + nu] - M[3 * 4 + nu];
            }
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                Y[a][0] = T[a][0] + T[a][1] + T[a][2];
                Y[a][1] = T[a][1] - T[a][2] - T[a][3];
            }
        }
        SNNHIP_STAMP(4);
        // ---- epilogue: bias/BN/act, tanh; channel 2*dy+dx of input pixel (yy, xx) -> output pixel (2yy+dy, 2xx+dx)
        // (depth_to_space, fs_subpixel.glsl:41-64): the tile's 2x2 pixels x 4 channels are a 4x4 block of the output image
        float* yn = y + static_cast<size_t>(n) * (2 * p.H) * (2 * p.W);
        const int gy0 = y0 + 2 * trow, gx0 = x0 + 2 * tcol;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                float o[4];
#pragma unroll
                for (int bb = 0; bb < 2; ++bb)
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        const int oc = 2 * dy + dx;
                        o[2 * bb + dx] = fast_tanh(apply_act<SIMPLE>(p.act, fmaf(Y[a][bb][oc], sc[oc], sh[oc]), 0.0f));
                    }
                const int gy = gy0 + a;
                float* row = yn + static_cast<size_t>(2 * gy + dy) * (2 * p.W) + 2 * gx0;
                if (gy < p.H) {
                    if (gx0 + 1 < p.W) {
                        *reinterpret_cast<float4*>(row) = make_float4(o[0], o[1], o[2], o[3]);
                    } else if (gx0 < p.W) {
                        *reinterpret_cast<float2*>(row) = make_float2(o[0], o[1]);
                    }
                }
            }
        SNNHIP_STAMP(5);
        if (!more) break;
        __syncthreads(); // the last quad of the next tile is in place
        tile = next;
    }
    SNNHIP_STAMP(6);
}

// ---- the launch sites: one function template per kernel over its compile-time parameters; the frame end (FrameIn / FrameOut, espcn_common.h) picks
// the kernel and becomes that kernel's own parameter block here
template <int K1, int AM>
void launch_a_wino(hipStream_t stream, dim3 grid, const FusedAParams& p, const FrameIn& f, const void* x, const float* w1, const float* w2, const float* ep1,
                   const float* ep2, float* y, hipEvent_t evStart, hipEvent_t evStop) {
    if (f.bits == 16)
        SNNHIP_LAUNCH_EV((conv_kxk_c1o16_wino3x3_c16o16_u16_kernel<K1, W_TH, AM, W_WPS>), grid, dim3(256), 0, stream, evStart, evStop, p,
                         U16InCfg{f.mean, f.norm, f.shift}, static_cast<const unsigned short*>(x), w1, w2, ep1, ep2, y);
    else if (f.bits == 8)
        SNNHIP_LAUNCH_EV((conv_kxk_c1o16_wino3x3_c16o16_u8_kernel<K1, W_TH, AM, W_WPS>), grid, dim3(256), 0, stream, evStart, evStop, p,
                         U8InCfg{f.mean, f.norm}, static_cast<const unsigned char*>(x), w1, w2, ep1, ep2, y);
    else
        SNNHIP_LAUNCH_EV((conv_kxk_c1o16_wino3x3_c16o16_kernel<K1, W_TH, AM, W_WPS>), grid, dim3(256), 0, stream, evStart, evStop, p,
                         static_cast<const float*>(x), w1, w2, ep1, ep2, y);
}

template <int K1, bool S>
void launch_a_direct(hipStream_t stream, dim3 grid, const FusedAParams& p, const float* x, const float* w1, const float* w2, const float* ep1, const float* ep2,
                     float* y, hipEvent_t evStart, hipEvent_t evStop) {
    SNNHIP_LAUNCH_EV((conv_kxk_c1o16_conv3x3_c16o16_kernel<K1, A_TW, A_TH, S>), grid, dim3(256), 0, stream, evStart, evStop, p, x, w1, w2, ep1, ep2, y);
}

template <bool S>
void launch_b_valu(hipStream_t stream, dim3 grid, const FusedBParams& p, const FrameOut& f, const float* x, const float* w, const float* ep, void* y,
                   hipEvent_t evStart, hipEvent_t evStop) {
    if (f.bits == 16)
        SNNHIP_LAUNCH_EV((conv3x3_c16o4_d2s_tanh_u16_kernel<B_TW, B_TH, S>), grid, dim3(256), 0, stream, evStart, evStop, p,
                         U16OutCfg{f.scale, f.offset, f.maxval, f.shift}, x, w, ep, static_cast<unsigned short*>(y));
    else if (f.bits == 8)
        SNNHIP_LAUNCH_EV((conv3x3_c16o4_d2s_tanh_u8_kernel<B_TW, B_TH, S>), grid, dim3(256), 0, stream, evStart, evStop, p, U8OutCfg{f.scale, f.offset}, x, w, ep,
                         static_cast<unsigned char*>(y));
    else
        SNNHIP_LAUNCH_EV((conv3x3_c16o4_d2s_tanh_kernel<B_TW, B_TH, S>), grid, dim3(256), 0, stream, evStart, evStop, p, x, w, ep, static_cast<float*>(y));
}

} // namespace

int espcn_fused_a_launch(hipStream_t stream, const FusedAParams& p, int k1, bool wino, const FrameIn& f, int computeUnits, const void* x, const float* w1,
                         const float* w2, const float* ep1, const float* ep2, float* y, hipEvent_t evStart, hipEvent_t evStop) {
    SNNHIP_REQUIRE(f.bits == 0 || espcn_fused_a_takes_frame(wino), "espcn_fused_a: the direct form takes no %d-bit frame", f.bits);
    const int ntiles = p.tilesX * p.tilesY * p.N;
    const bool simple = act_is_simple(p.act1.act) && act_is_simple(p.act2.act);
    if (wino) {
        const int slots = W_WPS * (computeUnits > 0 ? computeUnits : 256);
        const dim3 grid(ntiles < slots ? ntiles : slots); // persistent: W_WPS blocks per CU walk the tile list
        const int am = (p.act1.act == SNNHIP_ACT_RELU && p.act2.act == SNNHIP_ACT_RELU) ? 2 : (simple ? 1 : 0);
        if (k1 == 5) {
            if (am == 2) launch_a_wino<5, 2>(stream, grid, p, f, x, w1, w2, ep1, ep2, y, evStart, evStop);
            else if (am == 1) launch_a_wino<5, 1>(stream, grid, p, f, x, w1, w2, ep1, ep2, y, evStart, evStop);
            else launch_a_wino<5, 0>(stream, grid, p, f, x, w1, w2, ep1, ep2, y, evStart, evStop);
        } else {
            if (am == 2) launch_a_wino<3, 2>(stream, grid, p, f, x, w1, w2, ep1, ep2, y, evStart, evStop);
            else if (am == 1) launch_a_wino<3, 1>(stream, grid, p, f, x, w1, w2, ep1, ep2, y, evStart, evStop);
            else launch_a_wino<3, 0>(stream, grid, p, f, x, w1, w2, ep1, ep2, y, evStart, evStop);
        }
    } else {
        const dim3 grid(ntiles);
        const float* x32 = static_cast<const float*>(x);
        if (k1 == 5) {
            if (simple) launch_a_direct<5, true>(stream, grid, p, x32, w1, w2, ep1, ep2, y, evStart, evStop);
            else launch_a_direct<5, false>(stream, grid, p, x32, w1, w2, ep1, ep2, y, evStart, evStop);
        } else {
            if (simple) launch_a_direct<3, true>(stream, grid, p, x32, w1, w2, ep1, ep2, y, evStart, evStop);
            else launch_a_direct<3, false>(stream, grid, p, x32, w1, w2, ep1, ep2, y, evStart, evStop);
        }
    }
    SNNHIP_CHECK_HIP(hipGetLastError());
    return SNNHIP_OK;
}

int espcn_fused_b_launch(hipStream_t stream, const FusedBParams& p, bool wino, const FrameOut& f, const float* x, const float* w, const float* ep, void* y,
                         hipEvent_t evStart, hipEvent_t evStop) {
    SNNHIP_REQUIRE(f.bits == 0 || espcn_fused_b_takes_frame(wino), "espcn_fused_b: the Winograd form writes no %d-bit frame", f.bits);
    const dim3 grid(p.tilesX * p.tilesY * p.N); // one block per tile
    const bool simple = act_is_simple(p.act.act);
    if (wino) {
        float* y32 = static_cast<float*>(y);
        if (simple) SNNHIP_LAUNCH_EV((conv3x3_c16o4_wino_d2s_tanh_kernel<true>), grid, dim3(256), 0, stream, evStart, evStop, p, x, w, ep, y32);
        else SNNHIP_LAUNCH_EV((conv3x3_c16o4_wino_d2s_tanh_kernel<false>), grid, dim3(256), 0, stream, evStart, evStop, p, x, w, ep, y32);
    } else if (simple) {
        launch_b_valu<true>(stream, grid, p, f, x, w, ep, y, evStart, evStop);
    } else {
        launch_b_valu<false>(stream, grid, p, f, x, w, ep, y, evStart, evStop);
    }
    SNNHIP_CHECK_HIP(hipGetLastError());
    return SNNHIP_OK;
}

std::vector<float> espcn_pack_conv1(const float* w_oihw, int k1, bool winoOrder) {
    const int taps = k1 * k1, ksteps = winoOrder ? wino_conv1_ksteps(k1) : (taps + 3) / 4;
    std::vector<float> img(static_cast<size_t>(ksteps) * 64, 0.0f);
    for (int s = 0; s < ksteps; ++s)
        for (int l = 0; l < 64; ++l) {
            const int t = winoOrder ? wino_conv1_tap(k1, s, l >> 4) : 4 * s + (l >> 4);
            if (t >= 0 && t < taps) img[s * 64 + l] = w_oihw[static_cast<size_t>(l & 15) * taps + t];
        }
    return img;
}

std::vector<float> espcn_pack_conv3x3_lanes(const float* w_oihw, int r) {
    std::vector<float> img(36 * 64, 0.0f);
    for (int row = 0; row < 16; ++row) {
        const int ch = r == 0 ? row : espcn_d2s_row_channel(r, row);
        if (ch < 0) continue;
        for (int tap = 0; tap < 9; ++tap)
            for (int ic = 0; ic < 16; ++ic) img[(tap * 4 + (ic & 3)) * 64 + (ic >> 2) * 16 + row] = w_oihw[(static_cast<size_t>(ch) * 16 + ic) * 9 + tap];
    }
    return img;
}

std::vector<float> espcn_pack_wino(const float* w_oihw, int OC) {
    static const double Gm[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    std::vector<float> img(static_cast<size_t>(OC) * 256, 0.0f);
    for (int oc = 0; oc < OC; ++oc)
        for (int ic = 0; ic < 16; ++ic) {
            const float* gk = w_oihw + (static_cast<size_t>(oc) * 16 + ic) * 9;
            double tmp[4][3];
            for (int xi = 0; xi < 4; ++xi)
                for (int v = 0; v < 3; ++v) tmp[xi][v] = Gm[xi][0] * gk[0 * 3 + v] + Gm[xi][1] * gk[1 * 3 + v] + Gm[xi][2] * gk[2 * 3 + v];
            for (int xi = 0; xi < 4; ++xi)
                for (int nu = 0; nu < 4; ++nu) {
                    const double u = tmp[xi][0] * Gm[nu][0] + tmp[xi][1] * Gm[nu][1] + tmp[xi][2] * Gm[nu][2];
                    const int pos = xi * 4 + nu, q = ic >> 2, slot = q ^ (((oc >> 2) & 1) << 1);
                    img[OC == 16 ? ((pos * 16 + oc) * 4 + slot) * 4 + (ic & 3) : ((pos * 4 + q) * 4 + oc) * 4 + (ic & 3)] = static_cast<float>(u);
                }
        }
    return img;
}

std::vector<float> espcn_pack_b_direct(const float* w_oihw) {
    std::vector<float> img(9 * 16 * 4);
    for (int tap = 0; tap < 9; ++tap)
        for (int ic = 0; ic < 16; ++ic)
            for (int o = 0; o < 4; ++o) img[(tap * 16 + ic) * 4 + o] = w_oihw[(static_cast<size_t>(o) * 16 + ic) * 9 + tap];
    return img;
}

std::vector<float> espcn_pack_stream_w3(const float* w_oihw) {
    std::vector<float> img(9 * 16 * 4);
    for (int dx = 0; dx < 3; ++dx)
        for (int ic = 0; ic < 16; ++ic)
            for (int dy = 0; dy < 3; ++dy)
                for (int o = 0; o < 4; ++o) img[(dx * 16 + ic) * 12 + dy * 4 + o] = w_oihw[(static_cast<size_t>(o) * 16 + ic) * 9 + dy * 3 + dx];
    return img;
}

std::vector<float> fold_epilogue(const std::vector<float>& epi4, int OC, int useBN, int r) {
    const int rows = r == 0 ? OC : 16;
    std::vector<float> out(static_cast<size_t>(rows) * 2, 0.0f);
    for (int row = 0; row < rows; ++row) {
        const int o = r == 0 ? row : espcn_d2s_row_channel(r, row);
        if (o < 0) continue;
        const float bias = epi4[o * 4 + 0], sc = epi4[o * 4 + 1], mean = epi4[o * 4 + 2], beta = epi4[o * 4 + 3];
        out[row * 2 + 0] = useBN ? sc : 1.0f;
        out[row * 2 + 1] = useBN ? sc * (bias - mean) + beta : bias;
    }
    return out;
}

} // namespace snnhip
