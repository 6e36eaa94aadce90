// frame_rgb_cbcr.h -- what the RGB -> 4:2:0 CbCr kernel of frame_rgb_cbcr.hip shares between its kernel, its plan and the coefficient table
// (include/snnhip.h: snnhip_rgb_cbcr_plan_create / snnhip_bicubic_taps_rgb420 / snnhip_rgb_cbcr_coefficients): the pattern of one upscale factor,
// the two chroma scales and the lane geometry.  The phase (bicubic_phase_ratio), the Keys cubic and the quantiser are frame_resample.h's; the luma
// of a pixel is frame_colour.h's, the one function rgb_luma and ycc_merge call.
#pragma once
#include "frame_colour.h"
#include "frame_resample.h"

namespace snnhip {

// The output chroma grid has r / 2 samples per low-resolution pixel.  With g = gcd(r, 2) the pattern repeats every P = r / g outputs over S = 2 / g
// inputs: output P x' + p reads low-resolution position S x' + s_p, s_p = (2p + lead) / r - 0.5.  (P, S) = (1, 1), (3, 2), (2, 1) for r = 2, 3, 4.
constexpr int rgb420_phases(int r) { return r % 2 ? r : r / 2; }
constexpr int rgb420_step(int r) { return r % 2 ? 2 : 1; }
// where output chroma sample I sits between output luma columns 2I and 2I + 1, in luma columns from the left edge of column 2I
inline double rgb420_lead(int siting) { return siting == SNNHIP_SITING_LEFT ? 0.5 : 1.0; }

// Full-range differences dB = B - ylo, dR = R - ylo to Cb, Cr codes: Coff and the two scales, computed in double and rounded to float.  cbs and crs
// are the inverses of yuv_rgb's cbu and crv at maxval 255.
struct RgbCbcrCoeffs {
    float coff, cbs, crs;
};
inline RgbCbcrCoeffs rgb_cbcr_coeffs(int range, double kr, double kb) {
#pragma clang fp contract(off)
    const double crange = range == SNNHIP_RANGE_LIMITED ? 224.0 : 255.0;
    RgbCbcrCoeffs c;
    c.coff = 128.0f;
    c.cbs = static_cast<float>(crange / (2.0 * (1.0 - kb) * 255.0));
    c.crs = static_cast<float>(crange / (2.0 * (1.0 - kr) * 255.0));
    return c;
}

// One lane of the kernel owns kCbcrIn low-resolution pixels of a row -- K = kCbcrIn / S periods of the pattern -- and the P * K output chroma pixels
// over them (8, 12 or 16 bytes of CbCr for r = 2, 3, 4) in each output row of its wave.  A wave is 64 lanes side by side and marches down T periods of
// the vertical pattern: S * T + 4 low-resolution rows in, P * T output rows out.  A block is four waves one above the other.
constexpr int kCbcrIn = 4;    // low-resolution pixels per lane and row
constexpr int kCbcrWaves = 4; // waves per block
template <int R>
struct CbcrGeom {
    static constexpr int P = rgb420_phases(R);
    static constexpr int S = rgb420_step(R);
    static constexpr int K = kCbcrIn / S;       // periods per lane
    static constexpr int T = R == 2 ? 2 : 1;    // vertical periods per wave (r = 2: one output row per period, so two of them share four of their rows)
    static constexpr int TAPS = S + 4;          // weights of a phase over offsets -2 .. S + 1 from S x' (base -1 .. 1 folded in; S = 1 never has base 1)
    static constexpr int NB = kCbcrIn + 4;      // staged pixels per lane and row: two pixels of apron either side
    static constexpr int ROWS = S * T + 4;      // staged rows per wave
    static constexpr int OPX = P * K;           // output chroma pixels per lane and output row
    static constexpr int OW = OPX * 2 / 4;      // ... dwords
    static constexpr int OROWS = P * T;         // output rows per wave
    static constexpr int TILE_H = OROWS * kCbcrWaves; // in output chroma pixels
    static constexpr int TILE_W = 64 * OPX;
    static_assert(K * S == kCbcrIn && OPX * 2 == OW * 4, "a lane owns whole periods and whole dwords of output");
};

inline void rgb_cbcr_tile(int r, int* th, int* tw) {
    const int p = rgb420_phases(r), s = rgb420_step(r);
    *th = p * (r == 2 ? 2 : 1) * kCbcrWaves;
    *tw = 64 * p * (kCbcrIn / s);
}

} // namespace snnhip
