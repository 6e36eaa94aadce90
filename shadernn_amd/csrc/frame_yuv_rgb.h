// frame_yuv_rgb.h -- what the NV12 / P010 -> RGB kernel of frame_yuv_rgb.hip shares between its kernel, its plan and the coefficient table
// (include/snnhip.h: snnhip_yuv_rgb_plan_create / snnhip_bicubic_taps_420 / snnhip_yuv_rgb_coefficients): the matrix coefficients and the lane
// geometry of one (R, E) instance.  The phase of a resampling whose output grid is not the source's own (bicubic_phase_general, bicubic_phase_420),
// the Keys cubic and the quantiser are frame_resample.h's.
#pragma once
#include "frame_resample.h"

namespace snnhip {

// Y'CbCr -> full-range RGB at `maxval`: the offsets and the five coefficients of the contract, computed in double and rounded to float.
struct YuvRgbCoeffs {
    float yoff, coff;              // exact: multiples of (maxval + 1) / 256
    float cy, crv, cbu, cgv, cgu;
};
inline YuvRgbCoeffs yuv_rgb_coeffs(int maxval, int range, double kr, double kb) {
#pragma clang fp contract(off)
    const double k = (maxval + 1) / 256.0, m = maxval;
    const bool limited = range == SNNHIP_RANGE_LIMITED;
    const double yoff = limited ? 16.0 * k : 0.0, yrange = limited ? 219.0 * k : m, crange = limited ? 224.0 * k : m;
    const double kg = 1.0 - kr - kb;
    const double crv = 2.0 * (1.0 - kr) * m / crange, cbu = 2.0 * (1.0 - kb) * m / crange;
    YuvRgbCoeffs c;
    c.yoff = static_cast<float>(yoff);
    c.coff = static_cast<float>(128.0 * k);
    c.cy = static_cast<float>(m / yrange);
    c.crv = static_cast<float>(crv);
    c.cbu = static_cast<float>(cbu);
    c.cgv = static_cast<float>(kr * crv / kg);
    c.cgu = static_cast<float>(kb * cbu / kg);
    return c;
}

// One lane of the kernel owns 4 bytes of a chroma row (CP whole CbCr pixels: 2 of 8 bits, 1 of 16) and, in each of the 2r output rows under it, the
// 2r * CP output pixels they cover: 4r bytes of Yhi in, C * 4r bytes of RGB out.  A wave is 64 lanes side by side, a block four waves one above the
// other, each wave on one chroma row.
constexpr int kYuvWaves = 4; // waves (chroma rows) per block
template <int R, typename E>
struct YuvGeom {
    static constexpr int ES = static_cast<int>(sizeof(E));
    static constexpr int R2 = 2 * R;          // chroma -> output
    static constexpr int CP = 4 / (2 * ES);   // chroma pixels per lane
    static constexpr int NB = (CP + 4) * 2;   // staged chroma values per lane and row: two pixels of apron either side
    static constexpr int OPX = R2 * CP;       // output pixels per lane and output row
    static constexpr int YW = OPX * ES / 4;   // dwords of Yhi per lane and output row (= r)
    static constexpr int PER = 4 / ES;        // elements per dword
    static constexpr int TILE_H = kYuvWaves;
    static constexpr int TILE_W = 64 * CP;
    static_assert(OPX * ES == 4 * YW, "a lane reads whole dwords of Yhi");
};

inline void yuv_rgb_tile(int elemSize, int* th, int* tw) {
    *th = kYuvWaves;
    *tw = 64 * (4 / (2 * elemSize));
}

} // namespace snnhip
