// conv2d_upconv2.h -- tile constants and the host-side pre-summation of conv2d_upconv2.hip (nearest x2 UpSampling2D -> Conv2D 2x2 "same" on the
// low-resolution tensor).  The tests read the constants from this file.
#pragma once

namespace snnhip {

constexpr int kUpconv2TH = 8;   // low-resolution rows of a block tile (two per wave)
constexpr int kUpconv2TW = 16;  // low-resolution columns of a block tile = the MFMA's N
constexpr int kUpconv2OC = 32;  // output-channel granularity (a pair of 16-row MFMA blocks)
constexpr int kUpconv2ICBytes = 64; // input-channel granularity in bytes: 16 floats / 32 halfs, one LDS pixel
constexpr int kUpconv2Chain = 1152; // the longest run of terms one accumulator adds before it is flushed into a second one

// Per axis the three (phase, tap offset a) pairs that carry taps, in the order of snnhip_upconv2_presum_weights: e -> phase, a, first tap, tap count
// for pad offset p (0 or 1) on that axis: output coordinate 2 m + phase reads low-resolution index m - p + a.
inline void upconv2_axis_entry(int p, int e, int* phase, int* a, int* t0, int* nt) {
    // p = 1: (0, 0) <- tap 0; (0, 1) <- tap 1; (1, 1) <- taps 0 + 1.      p = 0: (0, 0) <- taps 0 + 1; (1, 0) <- tap 0; (1, 1) <- tap 1.
    static const int tab[2][3][4] = {{{0, 0, 0, 2}, {1, 0, 0, 1}, {1, 1, 1, 1}}, {{0, 0, 0, 1}, {0, 1, 1, 1}, {1, 1, 0, 2}}};
    *phase = tab[p][e][0]; *a = tab[p][e][1]; *t0 = tab[p][e][2]; *nt = tab[p][e][3];
}

// out[(3 ey + ex)][oc][ic] = the sum, in fp32 and in tap order (row-major), of the taps of entry (ey, ex); rowPad / colPad = the near pad of the rows / columns
inline void upconv2_presum(const float* w_oihw, int OC, int IC, int rowPad, int colPad, float* out) {
    for (int ey = 0; ey < 3; ++ey)
        for (int ex = 0; ex < 3; ++ex) {
            int ph, a, ty0, nty, tx0, ntx;
            upconv2_axis_entry(rowPad, ey, &ph, &a, &ty0, &nty);
            upconv2_axis_entry(colPad, ex, &ph, &a, &tx0, &ntx);
            float* dst = out + static_cast<size_t>(3 * ey + ex) * OC * IC;
            for (size_t i = 0; i < static_cast<size_t>(OC) * IC; ++i) {
                float s = 0.0f;
                for (int ty = ty0; ty < ty0 + nty; ++ty)
                    for (int tx = tx0; tx < tx0 + ntx; ++tx) s += w_oihw[i * 4 + ty * 2 + tx];
                dst[i] = s;
            }
        }
}

} // namespace snnhip
