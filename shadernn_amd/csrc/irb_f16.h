// irb_f16.h -- tile constants and host-side weight packing of irb_f16.hip (chain rule G on half tensors).
#pragma once

#include <cstddef>
#include <vector>

namespace snnhip {
namespace irb_f16 {

constexpr int kTile = 8;        // output tile of a block: 8 x 8 pixels, one 16-pixel group (two tile rows) per wave
constexpr int kSlice = 32;      // hidden channels per slice = one K-step of the projection's v_mfma_f32_16x16x32_f16
constexpr int kKStep = 32;      // input channels per K-step of the expand MFMAs
constexpr int kHPitch = 40;     // halves per halo pixel of a hidden slice tile: 32 + 8 (80 bytes: consecutive pixels start 5 16-byte slots apart)
constexpr int kMaxC = 160;      // five K-steps of expand weights in a lane's registers
constexpr int kMaxCo = 320;     // twenty accumulator tiles = 80 registers
constexpr size_t kMaxLds = 160 * 1024;
constexpr int kDwSliceFloats = 9 * kSlice + 2 * kSlice; // per slice: [tap][32] depthwise weights, scale[32], shift[32]

inline int halo(int stride) { return (kTile - 1) * stride + 3; }                    // 10 | 17
inline int x_pitch(int C) { return (C + kKStep - 1) / kKStep * kKStep + 8; }        // halves per halo pixel of the x tile (an odd number of 16-byte slots)
inline size_t lds_bytes(int C, int stride) {
    const int npx = (halo(stride) * halo(stride) + 15) / 16 * 16;
    return static_cast<size_t>(npx) * (x_pitch(C) * 2 + 2 * kHPitch * 2 + 4); // x tile, two hidden slice tiles, the in-image mask
}

// (scale, shift) per channel so that epilogue = act(acc * scale + shift), from the layer's {bias, bnScale, bnMean, bnBeta} table
inline void fold(const std::vector<float>& epi4, int c, int useBN, float* scale, float* shift) {
    const float bias = epi4[c * 4 + 0], sc = epi4[c * 4 + 1], mean = epi4[c * 4 + 2], beta = epi4[c * 4 + 3];
    *scale = useBN ? sc : 1.0f;
    *shift = useBN ? sc * (bias - mean) + beta : bias;
}

// Everything below is zero past C / Ch / Co: a padded hidden channel is act(0 * acc + 0) = 0 through all three stages.
//
// expand A operands: [slice][m tile 0 | 1][K-step][lane = 16 kg + m] 8 halves {We[32 slice + 16 mt + m][32 ks + 8 kg + i]}: the layout a lane of
// v_mfma_f32_16x16x32_f16 holds (row m, K values 8 kg .. 8 kg + 7), converted as the fp16 convolution plans convert (round to nearest even)
inline std::vector<_Float16> pack_expand(const std::vector<float>& w /* [Ch][C] */, int C, int Ch) {
    const int KS = (C + kKStep - 1) / kKStep, nS = (Ch + kSlice - 1) / kSlice;
    std::vector<_Float16> out(static_cast<size_t>(nS) * 2 * KS * 64 * 8, static_cast<_Float16>(0.0f));
    for (int hc = 0; hc < Ch; ++hc)
        for (int ic = 0; ic < C; ++ic) {
            const int j = hc / kSlice, mt = (hc % kSlice) / 16, m = hc % 16, ks = ic / kKStep, kg = (ic % kKStep) / 8, i = ic % 8;
            out[((static_cast<size_t>(j * 2 + mt) * KS + ks) * 64 + kg * 16 + m) * 8 + i] = static_cast<_Float16>(w[static_cast<size_t>(hc) * C + ic]);
        }
    return out;
}
// expand epilogue: [slice][m tile][scale x 16 | shift x 16] (a lane's four accumulator rows are channels 4 g .. 4 g + 3 of the m tile: one float4 each)
inline std::vector<float> pack_expand_epi(const std::vector<float>& epi4, int Ch, int useBN) {
    const int nS = (Ch + kSlice - 1) / kSlice;
    std::vector<float> out(static_cast<size_t>(nS) * 64, 0.0f);
    for (int hc = 0; hc < Ch; ++hc) fold(epi4, hc, useBN, &out[(hc / 16) * 32 + hc % 16], &out[(hc / 16) * 32 + 16 + hc % 16]);
    return out;
}
// depthwise: fp32 weights (what depthwise.hip multiplies half tensors by) [slice][tap][32], then scale[32], shift[32]
inline std::vector<float> pack_depthwise(const std::vector<float>& w /* [Ch][9] */, const std::vector<float>& epi4, int Ch, int useBN) {
    const int nS = (Ch + kSlice - 1) / kSlice;
    std::vector<float> out(static_cast<size_t>(nS) * kDwSliceFloats, 0.0f);
    for (int hc = 0; hc < Ch; ++hc) {
        float* s = out.data() + static_cast<size_t>(hc / kSlice) * kDwSliceFloats;
        for (int t = 0; t < 9; ++t) s[t * kSlice + hc % kSlice] = w[static_cast<size_t>(hc) * 9 + t];
        fold(epi4, hc, useBN, &s[9 * kSlice + hc % kSlice], &s[10 * kSlice + hc % kSlice]);
    }
    return out;
}
// project A operands: [slice][output block cb][lane = 16 kg + m] 8 halves {Wp[16 cb + m][32 slice + 8 kg + i]}
inline std::vector<_Float16> pack_project(const std::vector<float>& w /* [Co][Ch] */, int Ch, int Co) {
    const int nS = (Ch + kSlice - 1) / kSlice, NCB = (Co + 15) / 16;
    std::vector<_Float16> out(static_cast<size_t>(nS) * NCB * 64 * 8, static_cast<_Float16>(0.0f));
    for (int co = 0; co < Co; ++co)
        for (int hc = 0; hc < Ch; ++hc) {
            const int j = hc / kSlice, kg = (hc % kSlice) / 8, i = hc % 8;
            out[((static_cast<size_t>(j) * NCB + co / 16) * 64 + kg * 16 + co % 16) * 8 + i] = static_cast<_Float16>(w[static_cast<size_t>(co) * Ch + hc]);
        }
    return out;
}
// project epilogue: [output block][scale x 16 | shift x 16]
inline std::vector<float> pack_project_epi(const std::vector<float>& epi4, int Co, int useBN) {
    const int NCB = (Co + 15) / 16;
    std::vector<float> out(static_cast<size_t>(NCB) * 32, 0.0f);
    for (int co = 0; co < Co; ++co) fold(epi4, co, useBN, &out[(co / 16) * 32 + co % 16], &out[(co / 16) * 32 + 16 + co % 16]);
    return out;
}

} // namespace irb_f16
} // namespace snnhip
