// espcn_f16.hip -- the fp16 ESPCN chain in two launches on the f16 matrix cores (v_mfma_f32_16x16x32_f16 / v_mfma_f32_16x16x16_f16), opt-in with
// SNNHIP_ESPCN_F16=1; the rules themselves (pattern match, cost) are in the chain planner, chain_fuse.hip.  DESIGN.md section 4.11.
//
//   kernel A16     conv k x k (1 -> 16, k = 3 or 5) + act -> conv 3x3 (16 -> 16) + act          fp16 [N,H,W,1] (or an 8-bit frame) -> fp16 [N,H,W,16]
//   kernel B16<R>  conv 3x3 (16 -> R*R) + act -> depth-to-space(R) + tanh,  R = 2, 3, 4          fp16 [N,H,W,16] -> fp16 [N,R*H,R*W,1] (or an 8-bit frame)
//
// Quantisation points = those of the per-layer fp16 plans: fp16 weights and inputs, fp16 x fp16 products accumulated in fp32, bias / BN / act in
// fp32, one round-to-nearest-even to fp16 behind conv1 (into LDS), conv2 (the intermediate tensor), conv3 + act (a register) and tanh.
//
// Both kernels run their 3x3 convolution with 16 input channels from an LDS tile [row][col][16 ch] of halfs, 32 B per pixel = two 16-byte slots
// (channels 0..7 | 8..15), the slots swapped where bit 2 of the pixel's column is set.  The GEMM is D[row][pixel] += Wt[row][k] * X[k][pixel] with K
// ordered tap-major, channel-minor (k = 16*tap + ic): K-step s of the 16x16x32 form covers taps 2s and 2s+1, lane (px = lane & 15, g = lane >> 4)
// supplies k = 8g .. 8g+7 = channels 8(g & 1) .. of tap 2s + (g >> 1) at pixel px -- one ds_read_b128 -- and the ninth tap takes one 16x16x16 step
// (channels 4g .. 4g+3: one ds_read_b64).  Per 16 pixels: 5 MFMAs and 5 LDS reads where the fp32 kernels issue 36 and 9.  The ds_read_b128 lane
// groups ({0-3, 12-15, 20-27}, ...) see 16 distinct (pixel mod 8, slot) pairs: conflict-free for every tap shift; the slot swap is for the
// 8-byte stores of conv1's epilogue (lanes px and px + 4 would share banks without it).
//
// Alignment: fp16 tensors are 16-byte aligned at their base (snnhip_tensor_alloc / _wrap), so the 16-channel tensors take 16- and 8-byte accesses;
// the 1-channel ends are only 2-byte aligned per row: A16 loads single elements, B16<2> / <4> store one run of R halfs per lane (4 / 8 bytes, aligned
// because R*W and R*x are multiples of R), B16<3> stores 6 bytes as 4 + 2 or 2 + 4 by the parity of its address.
#include <hip/hip_ext.h>

#include <cstdint>

#include "espcn_f16.h"
#include "snnhip_internal.h"

namespace snnhip {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// the A operand of a 3x3 convolution with 16 input channels (espcn_f16_pack_w3's image): 18 VGPRs, held for the whole kernel
struct W3Regs {
    f16x8 a[4];
    f16x4 last;
};
__device__ __forceinline__ W3Regs load_w3(const _Float16* __restrict__ w, int lane) {
    W3Regs r;
#pragma unroll
    for (int s = 0; s < 4; ++s) r.a[s] = *reinterpret_cast<const f16x8*>(w + (s * 64 + lane) * 8);
    r.last = *reinterpret_cast<const f16x4*>(w + 4 * 64 * 8 + lane * 4);
    return r;
}

// half offset of 16-byte slot h (channels 8h ..) inside the pixel at tile column c
__device__ __forceinline__ int slot_off(int h, int c) { return (h ^ ((c >> 2) & 1)) * 8; }

// conv 3x3 (16 -> 16 rows) for G groups of 16 pixels of one wave: group gi = row row0 + gi / GPR, columns 16 * (gi % GPR) .. + 15 of the output
// tile; `tile` is the halo tile (origin one pixel up and left), PITCH pixels per row.  G independent accumulation chains.
template <int G, int GPR, int PITCH>
__device__ __forceinline__ void conv3x3_c16_tile(const _Float16* tile, int row0, int px, int g, const W3Regs& w, f32x4 (&acc)[G]) {
    const _Float16* base = tile + row0 * PITCH * 16;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int tap = 2 * s + (g >> 1), fy = tap / 3, fx = tap - 3 * fy, c = px + fx; // (16 * (gi % GPR) does not touch bit 2 of the column)
        const int off = (fy * PITCH + c) * 16 + slot_off(g & 1, c);
        f16x8 b[G];
#pragma unroll
        for (int gi = 0; gi < G; ++gi) b[gi] = *reinterpret_cast<const f16x8*>(base + ((gi / GPR) * PITCH + (gi % GPR) * 16) * 16 + off);
#pragma unroll
        for (int gi = 0; gi < G; ++gi) acc[gi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.a[s], b[gi], acc[gi], 0, 0, 0);
    }
    {
        const int c = px + 2;
        const int off = (2 * PITCH + c) * 16 + slot_off(g >> 1, c) + (g & 1) * 4;
        f16x4 b[G];
#pragma unroll
        for (int gi = 0; gi < G; ++gi) b[gi] = *reinterpret_cast<const f16x4*>(base + ((gi / GPR) * PITCH + (gi % GPR) * 16) * 16 + off);
#pragma unroll
        for (int gi = 0; gi < G; ++gi) acc[gi] = __builtin_amdgcn_mfma_f32_16x16x16f16(w.last, b[gi], acc[gi], 0, 0, 0);
    }
}

// ---- kernel A16 (TIn = _Float16) and its 8-bit form (TIn = unsigned char: the frame is normalised while the tile is staged,
// half((float(u) - mean) * norm), snnhip_u8_in_plan_create's fp16 map; a tap outside the image is 0 in the normalised domain)
template <int K1, typename TIn, bool SIMPLE>
__global__ __launch_bounds__(256) void espcn_f16_conv_pair_kernel(EspcnF16AParams p, const TIn* __restrict__ x, const _Float16* __restrict__ w1,
                                                                 const _Float16* __restrict__ w2, const float* __restrict__ ep1,
                                                                 const float* __restrict__ ep2, _Float16* __restrict__ y) {
    constexpr U16InCfg qin16{0.0f, 0.0f, 0};
#include "espcn_f16_a_body.h"
}

// the 16-bit frame form of kernel A16 (snnhip_u16_in_plan_create folded in): a parameter block of its own
template <int K1, bool SIMPLE>
__global__ __launch_bounds__(256) void espcn_f16_conv_pair_u16_kernel(EspcnF16AParams p, U16InCfg qin16, const unsigned short* __restrict__ x,
                                                                     const _Float16* __restrict__ w1, const _Float16* __restrict__ w2,
                                                                     const float* __restrict__ ep1, const float* __restrict__ ep2, _Float16* __restrict__ y) {
    typedef unsigned short TIn;
#include "espcn_f16_a_body.h"
}

// ---- kernel B16<R> (TOut = _Float16) and its 8-bit form (TOut = unsigned char: q = quantize_u8(float(half(tanh)), qscale, qoffset),
// snnhip_u8_out_plan_create's map on the fp16 value the stand-alone chain would have stored).  The 16 MFMA rows are not the channels in order:
// row 4*dy + dx holds channel R*dy + dx (espcn_d2s_row_channel), so lane (px, g < R) ends up with the R consecutive pixels of output row R*y + g
// that its low-resolution pixel owns and the 16 lanes of one g hold 16*R consecutive pixels of that row (espcn_d2s_mfma_body.h).
template <int R, typename TOut, bool SIMPLE>
__global__ __launch_bounds__(256) void espcn_f16_d2s_kernel(EspcnF16BParams p, const _Float16* __restrict__ x, const _Float16* __restrict__ w,
                                                           const float* __restrict__ ep, TOut* __restrict__ y) {
    constexpr U16OutCfg qout16{0.0f, 0.0f, 0.0f, 0};
#include "espcn_f16_b_body.h"
}

// the 16-bit frame form of kernel B16<R> (snnhip_u16_out_plan_create folded in)
template <int R, bool SIMPLE>
__global__ __launch_bounds__(256) void espcn_f16_d2s_u16_kernel(EspcnF16BParams p, U16OutCfg qout16, const _Float16* __restrict__ x,
                                                               const _Float16* __restrict__ w, const float* __restrict__ ep, unsigned short* __restrict__ y) {
    typedef unsigned short TOut;
#include "espcn_f16_b_body.h"
}

// ---- the launch sites, as in espcn_f16_wide.hip.  The 8-bit forms keep their map in the kernel's parameter block: a stack copy of p takes it.
template <int K1, bool S>
int launch_a(hipStream_t stream, dim3 grid, EspcnF16AParams p, const FrameIn& f, const void* x, const _Float16* w1, const _Float16* w2, const float* ep1,
              const float* ep2, _Float16* y, hipEvent_t evStart, hipEvent_t evStop) {
    if (f.bits == 16) {
        SNNHIP_LAUNCH_EV((espcn_f16_conv_pair_u16_kernel<K1, S>), grid, dim3(256), 0, stream, evStart, evStop, p, U16InCfg{f.mean, f.norm, f.shift},
                         static_cast<const unsigned short*>(x), w1, w2, ep1, ep2, y);
    } else if (f.bits == 8) {
        p.mean = f.mean;
        p.norm = f.norm;
        SNNHIP_LAUNCH_EV((espcn_f16_conv_pair_kernel<K1, unsigned char, S>), grid, dim3(256), 0, stream, evStart, evStop, p, static_cast<const unsigned char*>(x), w1,
                         w2, ep1, ep2, y);
    } else {
        SNNHIP_LAUNCH_EV((espcn_f16_conv_pair_kernel<K1, _Float16, S>), grid, dim3(256), 0, stream, evStart, evStop, p, static_cast<const _Float16*>(x), w1, w2, ep1,
                         ep2, y);
    }
    SNNHIP_CHECK_HIP(hipGetLastError());
    return SNNHIP_OK;
}

template <int R, bool S>
int launch_b(hipStream_t stream, dim3 grid, EspcnF16BParams p, const FrameOut& f, const _Float16* x, const _Float16* w, const float* ep, void* y,
              hipEvent_t evStart, hipEvent_t evStop) {
    if (f.bits == 16) {
        SNNHIP_LAUNCH_EV((espcn_f16_d2s_u16_kernel<R, S>), grid, dim3(256), 0, stream, evStart, evStop, p, U16OutCfg{f.scale, f.offset, f.maxval, f.shift}, x, w, ep,
                         static_cast<unsigned short*>(y));
    } else if (f.bits == 8) {
        p.qscale = f.scale;
        p.qoffset = f.offset;
        SNNHIP_LAUNCH_EV((espcn_f16_d2s_kernel<R, unsigned char, S>), grid, dim3(256), 0, stream, evStart, evStop, p, x, w, ep, static_cast<unsigned char*>(y));
    } else {
        SNNHIP_LAUNCH_EV((espcn_f16_d2s_kernel<R, _Float16, S>), grid, dim3(256), 0, stream, evStart, evStop, p, x, w, ep, static_cast<_Float16*>(y));
    }
    SNNHIP_CHECK_HIP(hipGetLastError());
    return SNNHIP_OK;
}

} // namespace

void espcn_f16_pack_w3(const float* w_oihw, int r, _Float16* out) {
    for (int i = 0; i < kEspcnF16W3Halfs; ++i) out[i] = static_cast<_Float16>(0.0f);
    for (int lane = 0; lane < 64; ++lane) {
        const int row = lane & 15, g = lane >> 4;
        const int ch = r == 0 ? row : espcn_d2s_row_channel(r, row);
        if (ch < 0) continue;
        const float* wc = w_oihw + static_cast<size_t>(ch) * 16 * 9;
        for (int s = 0; s < 4; ++s)
            for (int j = 0; j < 8; ++j) out[(s * 64 + lane) * 8 + j] = static_cast<_Float16>(wc[(8 * (g & 1) + j) * 9 + 2 * s + (g >> 1)]);
        for (int j = 0; j < 4; ++j) out[4 * 64 * 8 + lane * 4 + j] = static_cast<_Float16>(wc[(4 * g + j) * 9 + 8]);
    }
}

void espcn_f16_pack_w1(const float* w_oihw, int k, _Float16* out) {
    for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
            const int t = 8 * (lane >> 4) + j;
            out[lane * 8 + j] = static_cast<_Float16>(t < k * k ? w_oihw[static_cast<size_t>(lane & 15) * k * k + t] : 0.0f);
        }
}

int espcn_f16_a_launch(hipStream_t stream, int k1, const EspcnF16AParams& p, const FrameIn& f, const void* x, const _Float16* w1, const _Float16* w2,
                       const float* ep1, const float* ep2, _Float16* y, hipEvent_t evStart, hipEvent_t evStop) {
    SNNHIP_REQUIRE(k1 == 3 || k1 == 5, "espcn_f16: first convolution %dx%d (3x3 or 5x5)", k1, k1);
    const dim3 grid(p.tilesX * p.tilesY * p.N);
    const bool simple = act_is_simple(p.act1.act) && act_is_simple(p.act2.act);
    if (k1 == 5)
        return simple ? launch_a<5, true>(stream, grid, p, f, x, w1, w2, ep1, ep2, y, evStart, evStop)
                      : launch_a<5, false>(stream, grid, p, f, x, w1, w2, ep1, ep2, y, evStart, evStop);
    return simple ? launch_a<3, true>(stream, grid, p, f, x, w1, w2, ep1, ep2, y, evStart, evStop)
                  : launch_a<3, false>(stream, grid, p, f, x, w1, w2, ep1, ep2, y, evStart, evStop);
}

int espcn_f16_b_launch(hipStream_t stream, int r, const EspcnF16BParams& p, const FrameOut& f, const _Float16* x, const _Float16* w, const float* ep, void* y,
                       hipEvent_t evStart, hipEvent_t evStop) {
    SNNHIP_REQUIRE(r >= 2 && r <= 4, "espcn_f16: upscale factor %d (2, 3 or 4)", r);
    const dim3 grid(p.tilesX * p.tilesY * p.N);
    const bool simple = act_is_simple(p.act.act);
    if (r == 2)
        return simple ? launch_b<2, true>(stream, grid, p, f, x, w, ep, y, evStart, evStop) : launch_b<2, false>(stream, grid, p, f, x, w, ep, y, evStart, evStop);
    if (r == 3)
        return simple ? launch_b<3, true>(stream, grid, p, f, x, w, ep, y, evStart, evStop) : launch_b<3, false>(stream, grid, p, f, x, w, ep, y, evStart, evStop);
    return simple ? launch_b<4, true>(stream, grid, p, f, x, w, ep, y, evStart, evStop) : launch_b<4, false>(stream, grid, p, f, x, w, ep, y, evStart, evStop);
}

} // namespace snnhip

extern "C" int snnhip_espcn_f16_pack_weights(const float* w_oihw, int ic, int k, int r, unsigned short* out, int capacity, int* count) {
    using namespace snnhip;
    SNNHIP_REQUIRE(w_oihw && out && count, "espcn_f16_pack_weights: null argument");
    SNNHIP_REQUIRE((ic == 1 && (k == 3 || k == 5)) || (ic == 16 && k == 3 && (r == 0 || (r >= 2 && r <= 4))),
                   "espcn_f16_pack_weights: ic=%d k=%d r=%d (1 -> 16 with k = 3 or 5; 16 -> 16 with r = 0; 16 -> r*r with r = 2, 3, 4)", ic, k, r);
    const int need = ic == 1 ? kEspcnF16W1Halfs : kEspcnF16W3Halfs;
    SNNHIP_REQUIRE(capacity >= need, "espcn_f16_pack_weights: %d halfs needed, room for %d", need, capacity);
    static_assert(sizeof(_Float16) == sizeof(unsigned short), "halfs are handed out as their bit patterns");
    if (ic == 1)
        espcn_f16_pack_w1(w_oihw, k, reinterpret_cast<_Float16*>(out));
    else
        espcn_f16_pack_w3(w_oihw, r, reinterpret_cast<_Float16*>(out));
    *count = need;
    return SNNHIP_OK;
}
