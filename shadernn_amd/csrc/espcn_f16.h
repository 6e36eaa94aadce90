// espcn_f16.h -- the fp16 ESPCN chain rules A16 / B16 (espcn_f16.hip): what the chain planner (chain_fuse.hip) needs to pack their weights and
// launch them.  Opt-in, SNNHIP_ESPCN_F16=1.  DESIGN.md section 4.11.
#pragma once
#include <hip/hip_runtime.h>

#include "epilogue.h"
#include "espcn_common.h"

namespace snnhip {

// low-resolution pixels per block (256 threads = 4 waves each)
constexpr int kEspcnF16TW_A = 32, kEspcnF16TH_A = 16; // kernel A16: a wave owns 4 rows x 2 column halves = 8 groups of 16 pixels
constexpr int kEspcnF16TW_B = 32, kEspcnF16TH_B = 8;  // kernel B16: a wave owns 2 rows x 2 column halves = 4 groups

// halfs of the A-operand image of a 3x3 convolution with 16 input channels and 16 MFMA rows: 4 K-steps of v_mfma_f32_16x16x32_f16 (taps 0..7)
// + 1 of v_mfma_f32_16x16x16_f16 (tap 8) = 16 x 16 x 9 values, none padded
constexpr int kEspcnF16W3Halfs = 4 * 64 * 8 + 64 * 4;
constexpr int kEspcnF16W1Halfs = 64 * 8; // conv1 (1 -> 16, up to 25 taps): one K-step of 32

// Lane-ordered fp16 A-operand image of a 3x3 convolution, K ordered tap-major, channel-minor (k = 16*tap + ic):
//   out[(s*64 + lane)*8 + j]   = W[ch(lane & 15)][ic = 8*(g & 1) + j][tap = 2*s + (g >> 1)]      s = 0..3, g = lane >> 4, j = 0..7
//   out[2048 + lane*4 + j]     = W[ch(lane & 15)][ic = 4*g + j][tap = 8]                          j = 0..3
// w_oihw is [OC][16][3][3] fp32 and is rounded to nearest even, as the fp16 convolution plans round their weights.  r = 0: row = output channel
// (OC = 16); r = 2, 3, 4: espcn_d2s_row_channel, espcn_common.h (OC = r*r).
void espcn_f16_pack_w3(const float* w_oihw, int r, _Float16* out);
// conv1 (1 -> 16, k x k, k*k <= 32): out[lane*8 + j] = W[oc = lane & 15][tap = 8*(lane >> 4) + j], zero from tap k*k on
void espcn_f16_pack_w1(const float* w_oihw, int k, _Float16* out);

struct EspcnF16AParams {
    int N, H, W, tilesX, tilesY; // input [N, H, W, 1], output [N, H, W, 16]; tiles of kEspcnF16TW_A x kEspcnF16TH_A
    ActCfg act1, act2;
    float mean, norm; // u8in: x = half((float(u) - mean) * norm)
};
struct EspcnF16BParams {
    int N, H, W, tilesX, tilesY; // input [N, H, W, 16], output [N, r*H, r*W, 1]; tiles of kEspcnF16TW_B x kEspcnF16TH_B
    ActCfg act;
    float qscale, qoffset; // u8out: q = quantize_u8(float(half(tanh)), qscale, qoffset)
};

// Kernel A16: Conv2D k1 x k1 (1 -> 16) + act -> Conv2D 3x3 (16 -> 16) + act on fp16 tensors, k1 = 3 or 5.  f: what x holds -- halfs, an 8-bit
// frame, half((float(u) - mean) * norm) (the launch writes the map into its copy of p), or a 16-bit one, half((float(u >> shift) - mean) * norm)
// (a U16InCfg block of its own).  w1 / w2: the images above; ep1 / ep2: 16 x {scale, shift} fp32.  evStart / evStop: a plan-profile event pair or null.
inline bool espcn_f16_takes_frame() { return true; } // kernels A16 and B16 read / write frames in their one form
int espcn_f16_a_launch(hipStream_t stream, int k1, const EspcnF16AParams& p, const FrameIn& f, const void* x, const _Float16* w1, const _Float16* w2,
                       const float* ep1, const float* ep2, _Float16* y, hipEvent_t evStart, hipEvent_t evStop);
// Kernel B16<r>: Conv2D 3x3 (16 -> r*r) + act -> depth-to-space(r) + tanh, r = 2, 3, 4.  f: what y takes -- halfs, an 8-bit frame (the map goes
// into the launch's copy of p), or a 16-bit one, quantize_u16(float(half(tanh)), scale, offset, maxval) << shift (a U16OutCfg block).  ep: 16 x
// {scale, shift} in MFMA row order.
int espcn_f16_b_launch(hipStream_t stream, int r, const EspcnF16BParams& p, const FrameOut& f, const _Float16* x, const _Float16* w, const float* ep, void* y,
                       hipEvent_t evStart, hipEvent_t evStop);

} // namespace snnhip
