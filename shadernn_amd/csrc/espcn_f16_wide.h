// espcn_f16_wide.h -- the fp16 ESPCN chain at the published widths, 1 -> 64 -> 32 -> r*r (espcn_f16_wide.hip): tile constants, weight images and
// launch entry points for the chain planner (chain_fuse.hip).  Opt-in with the narrow rules, SNNHIP_ESPCN_F16=1.  DESIGN.md section 4.21.
#pragma once
#include <hip/hip_runtime.h>

#include "espcn_f16.h"

namespace snnhip {

// the widths the kernels are instantiated for (both are template parameters of the kernels; see the static_asserts in espcn_f16_wide.hip)
constexpr int kEspcnF16WideC1 = 64, kEspcnF16WideC2 = 32;

// low-resolution pixels per block (256 threads = 4 waves each)
constexpr int kEspcnF16WideTW_A = 32, kEspcnF16WideTH_A = 8; // kernel A16 wide: a wave owns 2 rows x 2 column halves = 4 groups of 16 pixels x 2 row blocks
constexpr int kEspcnF16WideTW_B = 32, kEspcnF16WideTH_B = 8; // kernel B16 wide: a wave owns 2 rows x 2 column halves = 4 groups

// LDS of kernel A16 wide: the conv1 tile [TH+2][TW+2][C1] halfs (static, under 64 KB) -- the input tile is 2 * (TH+6) * (TW+6) bytes on top
constexpr int kEspcnF16WideLdsA = (kEspcnF16WideTH_A + 2) * (kEspcnF16WideTW_A + 2) * kEspcnF16WideC1 * 2;

// halfs of the A-operand image of a 3x3 convolution with IC input channels (a multiple of 32) and ROWS MFMA rows (a multiple of 16):
// 9 * IC / 32 K-steps of v_mfma_f32_16x16x32_f16, each one tap and 32 channels, none padded
constexpr int espcn_f16_wide_w3_halfs(int ic, int rows) { return 9 * ic * rows; }
constexpr int kEspcnF16WideW2Halfs = espcn_f16_wide_w3_halfs(kEspcnF16WideC1, kEspcnF16WideC2); // conv2: 18 K-steps x 2 row blocks
constexpr int kEspcnF16WideW3Halfs = espcn_f16_wide_w3_halfs(kEspcnF16WideC2, 16);              // conv3: 9 K-steps x 1 row block
constexpr int kEspcnF16WideW1Halfs = kEspcnF16WideC1 * 32;                                      // conv1: C1 rows x one K-step of 32 taps

// Lane-ordered fp16 A-operand image of a 3x3 convolution, K ordered tap-major, channel-minor (k = IC*tap + ic), K-step ks = tap * (IC/32) + ic/32,
// row block mb = row / 16 (MB = rows / 16 blocks):
//   out[((ks*MB + mb)*64 + lane)*8 + j] = W[ch(16*mb + lane%16)][ic = 32*(ks % (IC/32)) + 8*(lane/16) + j][tap = ks / (IC/32)]     j = 0..7
// w_oihw is [OC][IC][3][3] fp32, rounded to nearest even.  r = 0: row = output channel (OC = rows); r = 2, 3, 4: rows = 16, espcn_d2s_row_channel.
void espcn_f16_wide_pack_w3(const float* w_oihw, int ic, int rows, int r, _Float16* out);
// conv1 (1 -> C1, k x k, k*k <= 32): out[(mb*64 + lane)*8 + j] = W[oc = 16*mb + lane%16][tap = 8*(lane/16) + j], zero from tap k*k on
void espcn_f16_wide_pack_w1(const float* w_oihw, int c1, int k, _Float16* out);

// Kernel A16 wide: Conv2D k1 x k1 (1 -> 64) + act -> Conv2D 3x3 (64 -> 32) + act on fp16 tensors, k1 = 3 or 5.  The parameter blocks are the narrow
// kernels' (tiles of kEspcnF16WideTW_A x kEspcnF16WideTH_A).  f: what x holds -- halfs, an 8-bit frame (its map goes into the launch's copy of p) or a
// 16-bit one (a U16InCfg block), as kernel A16.  w1 / w2: the images above; ep1 / ep2: 64 / 32 x {scale, shift} fp32.
inline bool espcn_f16_wide_takes_frame() { return true; } // both kernels read / write frames in their one form
int espcn_f16_wide_a_launch(hipStream_t stream, int k1, const EspcnF16AParams& p, const FrameIn& f, const void* x, const _Float16* w1, const _Float16* w2,
                            const float* ep1, const float* ep2, _Float16* y, hipEvent_t evStart, hipEvent_t evStop);
// Kernel B16 wide<r>: Conv2D 3x3 (32 -> r*r) + act -> depth-to-space(r) + tanh, r = 2, 3, 4.  f: what y takes, as kernel B16.  ep: 16 x {scale,
// shift} in MFMA row order.
int espcn_f16_wide_b_launch(hipStream_t stream, int r, const EspcnF16BParams& p, const FrameOut& f, const _Float16* x, const _Float16* w, const float* ep, void* y,
                            hipEvent_t evStart, hipEvent_t evStop);

} // namespace snnhip
