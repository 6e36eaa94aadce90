// espcn_fused.h -- the fp32 ESPCN kernels A and B (espcn_fused.hip): what the chain planner (chain_fuse.hip) needs to pack their weights and launch
// them -- tile sizes, parameter blocks, the two launch functions and the host-side weight images (rule C's and rule B's r = 3 / 4 kernels, in units
// of their own, take images of the same families).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "epilogue.h"
#include "espcn_common.h"

namespace snnhip {

// Input-resolution pixels per block.  The values stand with the kernels they shape, at the top of espcn_fused.hip (the error-budget tests read them
// there); the planner needs them only at run time.
extern const int A_TW, A_TH;        // kernel A direct
extern const int W_TW, W_TH, W_WPS; // kernel A Winograd: tile W_TW (= WinoTile::TW) x W_TH, W_WPS blocks (waves/SIMD) per CU
extern const int B_TW, B_TH, BR_TW, BR_TH; // kernel B direct; its upscale 3 / 4 form (the tile of espcn_d2s_mfma.h)
extern const int BW_TW, BW_TH;      // kernel B Winograd

struct FusedAParams {
    int N, H, W, tilesX, tilesY;
    ActCfg act1, act2;
};
struct FusedBParams {
    int N, H, W, tilesX, tilesY;
    ActCfg act;
    unsigned magicX, magicY; // ceil(2^32 / tilesX), ceil(2^32 / tilesY): tile decode without integer division (exact for block ids < 2^16 * ...)
};
// the tile grid of an N x H x W input in tiles of tw x th, and its magic pair
inline FusedBParams espcn_b_params(int N, int H, int W, int tw, int th, const ActCfg& act) {
    const unsigned tx = static_cast<unsigned>((W + tw - 1) / tw), ty = static_cast<unsigned>((H + th - 1) / th);
    return FusedBParams{N, H, W, static_cast<int>(tx), static_cast<int>(ty), act, static_cast<unsigned>((0x100000000ull + tx - 1) / tx),
                        static_cast<unsigned>((0x100000000ull + ty - 1) / ty)};
}

// conv1 K-step -> tap assignment of the Winograd kernel: K-step s, lane group g (= MFMA k index) handle
//   s <  K1        : tap (row g, col s)            valid iff g < K1          -> LDS address = base + g*INW + s   (s is an immediate)
//   s == K1 + j    : tap (row 4, col 4j + g)       valid iff K1 == 5, col < 5 -> LDS address = base + 4*INW + g + 4j
// (invalid (s, g) carry a zero weight and read an initialised location).  Returns the tap index or -1.
inline int wino_conv1_tap(int K1, int s, int g) {
    if (s < K1) return g < K1 ? g * K1 + s : -1;
    const int col = 4 * (s - K1) + g;
    return (K1 > 4 && col < K1) ? 4 * K1 + col : -1;
}
constexpr int wino_conv1_ksteps(int K1) { return K1 + (K1 > 4 ? 2 : 0); }

// Kernel A: Conv2D k1 x k1 (1 -> 16) + act -> Conv2D 3x3 (16 -> 16) + act, k1 = 3 or 5.  wino: conv2 as Winograd F(2x2,3x3) on persistent blocks
// (W_WPS per compute unit; tiles of W_TW x W_TH), else direct (one block per A_TW x A_TH tile).  f: what x holds (floats, or an 8- / 16-bit
// frame).  w1 / w2: espcn_pack_conv1 + espcn_pack_wino (wino) or espcn_pack_conv3x3_lanes(., 0); ep1 / ep2: fold_epilogue.  evStart / evStop: a
// plan-profile event pair or null.
inline bool espcn_fused_a_takes_frame(bool wino) { return wino; } // only the Winograd form reads frames; the launch refuses any other
int espcn_fused_a_launch(hipStream_t stream, const FusedAParams& p, int k1, bool wino, const FrameIn& f, int computeUnits, const void* x, const float* w1,
                         const float* w2, const float* ep1, const float* ep2, float* y, hipEvent_t evStart, hipEvent_t evStop);
// Kernel B: Conv2D 3x3 (16 -> 4) + act -> depth-to-space(2) + tanh, one block per tile.  wino: the 4x4x1-MFMA Winograd form (BW_TW x BW_TH,
// w = espcn_pack_wino), else the VALU form (B_TW x B_TH, w = espcn_pack_b_direct).  f: what y takes (floats, or an 8- / 16-bit frame).
inline bool espcn_fused_b_takes_frame(bool wino) { return !wino; } // only the VALU form writes frames
int espcn_fused_b_launch(hipStream_t stream, const FusedBParams& p, bool wino, const FrameOut& f, const float* x, const float* w, const float* ep, void* y,
                         hipEvent_t evStart, hipEvent_t evStop);

// ---- host-side weight images; w_oihw = the convolution's [OC][IC][k][k] fp32 weights
// lane-ordered conv1 (1 -> 16, k1 x k1) A operand: image[s*64 + l] = W[oc = l & 15][tap], tap = 4s + l/16 (zero from k1*k1 on), or -- winoOrder --
// wino_conv1_tap(k1, s, l/16)
std::vector<float> espcn_pack_conv1(const float* w_oihw, int k1, bool winoOrder);
// lane-ordered 3x3 A operand with 16 input channels and 16 MFMA rows: image[(tap*4 + j)*64 + l] = W[ch(l & 15)][ic = 4*(l/16) + j][tap].  r = 0: row =
// output channel (16 -> 16); r = 3, 4 (16 -> r*r, rule B's kernel of espcn_d2s_mfma.hip): MFMA row 4*dy + dx <- channel r*dy + dx
// (espcn_d2s_row_channel; rows without a channel stay zero)
std::vector<float> espcn_pack_conv3x3_lanes(const float* w_oihw, int r);
// U[pos = xi*4+nu][oc][ic] = (G g Gt)[xi][nu] of every 3x3 filter, G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]], in double, stored as the LDS image of
//   kernel A (OC = 16): float4 index (pos*16 + oc)*4 + (q ^ 2*((oc>>2)&1)) holds ic = 4q .. 4q+3
//   kernel B (OC = 4):  float index ((pos*4 + ic/4)*4 + oc)*4 + ic%4
std::vector<float> espcn_pack_wino(const float* w_oihw, int OC);
// kernel B direct: image[(tap*16 + ic)*4 + o] = W[o][ic][tap]   (16 -> 4)
std::vector<float> espcn_pack_b_direct(const float* w_oihw);
// rule C's conv3: w3s[((dx*4+q)*4+i)*12 + dy*4 + o] = W3[o][ic = 4q+i][dy][dx]   (16 -> 4)
std::vector<float> espcn_pack_stream_w3(const float* w_oihw);
// (scale, shift) per channel so that epilogue = act(acc*scale + shift):  scale = bnScale, shift = bnScale*(bias-mean)+beta.  r = 0: OC rows in channel
// order; r = 2, 3, 4 (OC = r*r): 16 rows in the MFMA row order of a depth-to-space tail (espcn_d2s_row_channel), rows without a channel zero
std::vector<float> fold_epilogue(const std::vector<float>& epi4, int OC, int useBN, int r = 0);

} // namespace snnhip
