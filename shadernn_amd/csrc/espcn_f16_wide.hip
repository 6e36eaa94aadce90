// espcn_f16_wide.hip -- the fp16 ESPCN chain at the published widths (1 -> 64 -> 32 -> r*r) in two launches on the f16 matrix cores
// (v_mfma_f32_16x16x32_f16), opt-in with SNNHIP_ESPCN_F16=1 beside the 16-channel kernels of espcn_f16.hip; the rules are in the chain planner,
// chain_fuse.hip.  DESIGN.md section 4.21.
//
//   kernel A16 wide     conv k x k (1 -> C1, k = 3 or 5) + act -> conv 3x3 (C1 -> C2) + act      fp16 [N,H,W,1] (or an 8- / 16-bit frame) -> fp16 [N,H,W,C2]
//   kernel B16 wide<R>  conv 3x3 (C2 -> R*R) + act -> depth-to-space(R) + tanh,  R = 2, 3, 4      fp16 [N,H,W,C2] -> fp16 [N,R*H,R*W,1] (or a frame)
//
// C1 and C2 are template parameters; (64, 32) is what is instantiated.  Quantisation points = those of the per-layer fp16 plans, as in espcn_f16.hip.
//
// Both kernels run their 3x3 convolution from an LDS tile [row][col][C ch] of halfs: a pixel is C/8 16-byte slots (128 B in A's tile, 64 B in B's).
// The GEMM is D[row][pixel] += Wt[row][k] * X[k][pixel] with K ordered tap-major, channel-minor (k = C*tap + ic): K-step ks covers tap ks / (C/32),
// channels 32*(ks % (C/32)) .. + 31, and lane (px = lane & 15, g = lane >> 4) supplies the eight channels of slot 4*(ks % (C/32)) + g at pixel px
// shifted by the tap -- one ds_read_b128, which feeds C2/16 MFMAs (two row blocks in kernel A).  No 16x16x16 tail is left.
// Slot swizzle (wide_slot): a ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (+32): eight lanes of an even g
// and eight of g + 1, whose pixel sets are {0-3, 12-15} and {4-11} shifted by the tap, and 256 B = sixteen 16-byte bank units per cycle.
//   C = 64 (unit = 8*(col & 1) + slot):  slot' = slot ^ (((col >> 1) & 3) << 1).  Bit 0 of the slot keeps g and g + 1 apart; among the four
//           pixels of one parity in either set, (col >> 1) & 3 takes four values for every tap shift 0, 1, 2.
//   C = 32 (unit = 4*(col & 3) + slot):  slot' = slot ^ (((col >> 2) & 1) << 1): the two pixels of one residue mod 4 in either set differ in bit 2.
// So every lane group reads 16 distinct units: conflict-free for every tap.  A row step of the tile is a whole number of 128-byte halves
// (34 pixels), the same for all lanes.  The epilogue of A's phase 1 writes through the same map (8-byte stores of channels 16mb + 4g .. + 3: the
// 16 lanes of one store group land on 4 units, a 4-way conflict on 4 stores per 16 pixels beside 36 MFMAs -- accepted); B's staging writes whole
// slots (ds_write_b128).
//
// Tile of kernel A: 32 x 8 pixels, conv1 tile 10 x 34 x 64 halfs = 43 520 B of static LDS (+ the input tile, about 1 KB), so two to three blocks
// fit on a CU without a per-device attribute; the 32 x 16 tile (78 336 B, dynamic LDS) would halve the halo's share of conv1 (340 / 256 pixels
// -> 612 / 512) but leave one block per CU beside a second kernel.  conv2's A operand (36 KB of halfs) is held in registers: 36 f16x8 per lane.
#include <hip/hip_ext.h>

#include <cstdint>

#include "espcn_f16_wide.h"
#include "snnhip_internal.h"

namespace snnhip {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// physical 16-byte slot of logical slot s (channels 8s ..) inside the pixel at tile column c (see the header comment)
template <int C>
__device__ __forceinline__ int wide_slot(int s, int c) {
    static_assert(C == 32 || C == 64, "the slot swizzle is derived for 64- and 128-byte pixels");
    return C == 64 ? s ^ (((c >> 1) & 3) << 1) : s ^ (((c >> 2) & 1) << 1);
}

// conv 3x3 (C channels -> MB row blocks of 16) for G groups of 16 pixels of one wave: group gi = row row0 + gi / GPR, columns 16 * (gi % GPR) .. + 15
// of the output tile; `tile` is the halo tile (origin one pixel up and left), PITCH pixels per row.  G * MB independent accumulation chains.
template <int C, int MB, int G, int GPR, int PITCH>
__device__ __forceinline__ void conv3x3_wide_tile(const _Float16* tile, int row0, int px, int g, const f16x8 (&w)[9 * C / 32][MB], f32x4 (&acc)[G][MB]) {
    constexpr int KC = C / 32;
    const _Float16* base = tile + row0 * PITCH * C;
#pragma unroll
    for (int ks = 0; ks < 9 * KC; ++ks) {
        const int tap = ks / KC, ch = ks % KC, fy = tap / 3, fx = tap - 3 * fy, c = px + fx; // (16 * (gi % GPR) does not touch bits 0..3 of the column)
        const int off = (fy * PITCH + c) * C + wide_slot<C>(4 * ch + g, c) * 8;
        f16x8 b[G];
#pragma unroll
        for (int gi = 0; gi < G; ++gi) b[gi] = *reinterpret_cast<const f16x8*>(base + ((gi / GPR) * PITCH + (gi % GPR) * 16) * C + off);
#pragma unroll
        for (int gi = 0; gi < G; ++gi)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) acc[gi][mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[ks][mb], b[gi], acc[gi][mb], 0, 0, 0);
    }
}

// ---- kernel A16 wide (TIn = _Float16 or unsigned char) and its 16-bit frame form
template <int K1, int C1, int C2, typename TIn, bool SIMPLE>
__global__ __launch_bounds__(256) void espcn_f16_wide_conv_pair_kernel(EspcnF16AParams p, const TIn* __restrict__ x, const _Float16* __restrict__ w1,
                                                                      const _Float16* __restrict__ w2, const float* __restrict__ ep1,
                                                                      const float* __restrict__ ep2, _Float16* __restrict__ y) {
    constexpr U16InCfg qin16{0.0f, 0.0f, 0};
#include "espcn_f16_wide_a_body.h"
}

template <int K1, int C1, int C2, bool SIMPLE>
__global__ __launch_bounds__(256) void espcn_f16_wide_conv_pair_u16_kernel(EspcnF16AParams p, U16InCfg qin16, const unsigned short* __restrict__ x,
                                                                          const _Float16* __restrict__ w1, const _Float16* __restrict__ w2,
                                                                          const float* __restrict__ ep1, const float* __restrict__ ep2,
                                                                          _Float16* __restrict__ y) {
    typedef unsigned short TIn;
#include "espcn_f16_wide_a_body.h"
}

// ---- kernel B16 wide<R> (TOut = _Float16 or unsigned char) and its 16-bit frame form; MFMA rows as in kernel B16 (espcn_d2s_row_channel)
template <int R, int C2, typename TOut, bool SIMPLE>
__global__ __launch_bounds__(256) void espcn_f16_wide_d2s_kernel(EspcnF16BParams p, const _Float16* __restrict__ x, const _Float16* __restrict__ w,
                                                                const float* __restrict__ ep, TOut* __restrict__ y) {
    constexpr U16OutCfg qout16{0.0f, 0.0f, 0.0f, 0};
#include "espcn_f16_wide_b_body.h"
}

template <int R, int C2, bool SIMPLE>
__global__ __launch_bounds__(256) void espcn_f16_wide_d2s_u16_kernel(EspcnF16BParams p, U16OutCfg qout16, const _Float16* __restrict__ x,
                                                                    const _Float16* __restrict__ w, const float* __restrict__ ep,
                                                                    unsigned short* __restrict__ y) {
    typedef unsigned short TOut;
#include "espcn_f16_wide_b_body.h"
}

// ---- the launch sites.  The 8-bit forms keep their map in the kernel's parameter block: a stack copy of p takes it.
template <int K1, bool S>
int launch_a(hipStream_t stream, const dim3 grid, EspcnF16AParams p, const FrameIn& f, const void* x, const _Float16* w1, const _Float16* w2, const float* ep1,
             const float* ep2, _Float16* y, hipEvent_t evStart, hipEvent_t evStop) {
    constexpr int C1 = kEspcnF16WideC1, C2 = kEspcnF16WideC2;
    if (f.bits == 16) {
        SNNHIP_LAUNCH_EV((espcn_f16_wide_conv_pair_u16_kernel<K1, C1, C2, S>), grid, dim3(256), 0, stream, evStart, evStop, p, U16InCfg{f.mean, f.norm, f.shift},
                         static_cast<const unsigned short*>(x), w1, w2, ep1, ep2, y);
    } else if (f.bits == 8) {
        p.mean = f.mean;
        p.norm = f.norm;
        SNNHIP_LAUNCH_EV((espcn_f16_wide_conv_pair_kernel<K1, C1, C2, unsigned char, S>), grid, dim3(256), 0, stream, evStart, evStop, p,
                         static_cast<const unsigned char*>(x), w1, w2, ep1, ep2, y);
    } else {
        SNNHIP_LAUNCH_EV((espcn_f16_wide_conv_pair_kernel<K1, C1, C2, _Float16, S>), grid, dim3(256), 0, stream, evStart, evStop, p,
                         static_cast<const _Float16*>(x), w1, w2, ep1, ep2, y);
    }
    SNNHIP_CHECK_HIP(hipGetLastError());
    return SNNHIP_OK;
}

template <int R, bool S>
int launch_b(hipStream_t stream, const dim3 grid, EspcnF16BParams p, const FrameOut& f, const _Float16* x, const _Float16* w, const float* ep, void* y,
             hipEvent_t evStart, hipEvent_t evStop) {
    constexpr int C2 = kEspcnF16WideC2;
    if (f.bits == 16) {
        SNNHIP_LAUNCH_EV((espcn_f16_wide_d2s_u16_kernel<R, C2, S>), grid, dim3(256), 0, stream, evStart, evStop, p, U16OutCfg{f.scale, f.offset, f.maxval, f.shift},
                         x, w, ep, static_cast<unsigned short*>(y));
    } else if (f.bits == 8) {
        p.qscale = f.scale;
        p.qoffset = f.offset;
        SNNHIP_LAUNCH_EV((espcn_f16_wide_d2s_kernel<R, C2, unsigned char, S>), grid, dim3(256), 0, stream, evStart, evStop, p, x, w, ep,
                         static_cast<unsigned char*>(y));
    } else {
        SNNHIP_LAUNCH_EV((espcn_f16_wide_d2s_kernel<R, C2, _Float16, S>), grid, dim3(256), 0, stream, evStart, evStop, p, x, w, ep, static_cast<_Float16*>(y));
    }
    SNNHIP_CHECK_HIP(hipGetLastError());
    return SNNHIP_OK;
}

} // namespace

void espcn_f16_wide_pack_w3(const float* w_oihw, int ic, int rows, int r, _Float16* out) {
    const int kc = ic / 32, mbs = rows / 16;
    for (int ks = 0; ks < 9 * kc; ++ks)
        for (int mb = 0; mb < mbs; ++mb)
            for (int lane = 0; lane < 64; ++lane) {
                const int row = 16 * mb + (lane & 15), g = lane >> 4;
                const int ch = r == 0 ? row : espcn_d2s_row_channel(r, row);
                for (int j = 0; j < 8; ++j) {
                    const int c = 32 * (ks % kc) + 8 * g + j, tap = ks / kc;
                    out[((ks * mbs + mb) * 64 + lane) * 8 + j] = static_cast<_Float16>(ch < 0 ? 0.0f : w_oihw[(static_cast<size_t>(ch) * ic + c) * 9 + tap]);
                }
            }
}

void espcn_f16_wide_pack_w1(const float* w_oihw, int c1, int k, _Float16* out) {
    for (int mb = 0; mb < c1 / 16; ++mb)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j) {
                const int t = 8 * (lane >> 4) + j;
                out[(mb * 64 + lane) * 8 + j] = static_cast<_Float16>(t < k * k ? w_oihw[static_cast<size_t>(16 * mb + (lane & 15)) * k * k + t] : 0.0f);
            }
}

int espcn_f16_wide_a_launch(hipStream_t stream, int k1, const EspcnF16AParams& p, const FrameIn& f, const void* x, const _Float16* w1, const _Float16* w2,
                            const float* ep1, const float* ep2, _Float16* y, hipEvent_t evStart, hipEvent_t evStop) {
    SNNHIP_REQUIRE(k1 == 3 || k1 == 5, "espcn_f16_wide: first convolution %dx%d (3x3 or 5x5)", k1, k1);
    const dim3 grid(p.tilesX * p.tilesY * p.N);
    const bool simple = act_is_simple(p.act1.act) && act_is_simple(p.act2.act);
    if (k1 == 5)
        return simple ? launch_a<5, true>(stream, grid, p, f, x, w1, w2, ep1, ep2, y, evStart, evStop)
                      : launch_a<5, false>(stream, grid, p, f, x, w1, w2, ep1, ep2, y, evStart, evStop);
    return simple ? launch_a<3, true>(stream, grid, p, f, x, w1, w2, ep1, ep2, y, evStart, evStop)
                  : launch_a<3, false>(stream, grid, p, f, x, w1, w2, ep1, ep2, y, evStart, evStop);
}

int espcn_f16_wide_b_launch(hipStream_t stream, int r, const EspcnF16BParams& p, const FrameOut& f, const _Float16* x, const _Float16* w, const float* ep, void* y,
                            hipEvent_t evStart, hipEvent_t evStop) {
    SNNHIP_REQUIRE(r >= 2 && r <= 4, "espcn_f16_wide: upscale factor %d (2, 3 or 4)", r);
    const dim3 grid(p.tilesX * p.tilesY * p.N);
    const bool simple = act_is_simple(p.act.act);
    if (r == 2)
        return simple ? launch_b<2, true>(stream, grid, p, f, x, w, ep, y, evStart, evStop) : launch_b<2, false>(stream, grid, p, f, x, w, ep, y, evStart, evStop);
    if (r == 3)
        return simple ? launch_b<3, true>(stream, grid, p, f, x, w, ep, y, evStart, evStop) : launch_b<3, false>(stream, grid, p, f, x, w, ep, y, evStart, evStop);
    return simple ? launch_b<4, true>(stream, grid, p, f, x, w, ep, y, evStart, evStop) : launch_b<4, false>(stream, grid, p, f, x, w, ep, y, evStart, evStop);
}

} // namespace snnhip

extern "C" int snnhip_espcn_f16_wide_pack_weights(const float* w_oihw, int oc, int ic, int k, int r, unsigned short* out, int capacity, int* count) {
    using namespace snnhip;
    SNNHIP_REQUIRE(w_oihw && out && count, "espcn_f16_wide_pack_weights: null argument");
    const bool conv1 = ic == 1 && oc == kEspcnF16WideC1 && (k == 3 || k == 5) && r == 0;
    const bool conv2 = ic == kEspcnF16WideC1 && oc == kEspcnF16WideC2 && k == 3 && r == 0;
    const bool conv3 = ic == kEspcnF16WideC2 && k == 3 && r >= 2 && r <= 4 && oc == r * r;
    SNNHIP_REQUIRE(conv1 || conv2 || conv3,
                   "espcn_f16_wide_pack_weights: oc=%d ic=%d k=%d r=%d (1 -> %d with k = 3 or 5; %d -> %d with k = 3, r = 0; %d -> r*r with k = 3, r = 2, 3, 4)", oc,
                   ic, k, r, kEspcnF16WideC1, kEspcnF16WideC1, kEspcnF16WideC2, kEspcnF16WideC2);
    const int need = conv1 ? kEspcnF16WideW1Halfs : conv2 ? kEspcnF16WideW2Halfs : kEspcnF16WideW3Halfs;
    SNNHIP_REQUIRE(capacity >= need, "espcn_f16_wide_pack_weights: %d halfs needed, room for %d", need, capacity);
    static_assert(sizeof(_Float16) == sizeof(unsigned short), "halfs are handed out as their bit patterns");
    _Float16* o = reinterpret_cast<_Float16*>(out);
    if (conv1)
        espcn_f16_wide_pack_w1(w_oihw, oc, k, o);
    else if (conv2)
        espcn_f16_wide_pack_w3(w_oihw, ic, oc, 0, o);
    else
        espcn_f16_wide_pack_w3(w_oihw, ic, 16, r, o);
    *count = need;
    return SNNHIP_OK;
}
