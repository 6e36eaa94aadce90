// frame_chroma.h -- what the chroma-plane upsampler of frame_chroma.hip shares between its kernel and its plan (include/snnhip.h:
// snnhip_chroma_up_plan_create / snnhip_bicubic_taps_sited): the lane geometry of one (R, C, E) instance.  The sited phase (bicubic_phase_sited:
// centre s = (p + 0.5) / r - 0.5, left s = (p + 0.25) / r - 0.25), the Keys cubic and the quantiser are frame_resample.h's.
#pragma once
#include "frame_resample.h"

namespace snnhip {

// One lane of the kernel owns kIn bytes of an input row (a whole number of pixels) and R times as many bytes of each of the R output rows under it:
// 16 bytes out wherever R divides 16 (two such stores for 16-bit r = 4), 24 for r = 3.  A wave is 64 lanes side by side, a block four waves one above
// the other, each wave marching down kChromaRows input rows.
constexpr int kChromaRows = 2;  // input rows per wave (4 halves the loads per output row but leaves half the SIMDs of a 1080p frame without a wave)
constexpr int kChromaWaves = 4; // waves (row strips) per block
template <int R, int C, typename E>
struct ChromaGeom {
    static constexpr int ES = static_cast<int>(sizeof(E));
    static constexpr int IN = R == 1 ? 16 : (R == 4 && ES == 1 ? 4 : 8); // input bytes per lane and row
    static constexpr int NE = IN / ES;                                  // ... elements
    static constexpr int PX = NE / C;                                   // ... pixels
    static constexpr int AE = 2 * C;                                    // apron elements on each side (two pixels)
    static constexpr int NB = NE + 2 * AE;                              // staged values per lane and row
    static constexpr int NV = R * NE;                                   // output elements per lane and output row
    static constexpr int OUTB = NV * ES;                                // ... bytes: 16, 24 (r = 3) or 32 (16-bit r = 4)
    static constexpr int TILE_H = kChromaRows * kChromaWaves;
    static constexpr int TILE_W = 64 * PX;
    static_assert(PX >= 1 && PX * C == NE, "a lane owns whole pixels");
};

inline void chroma_tile(int r, int c, int elemSize, int* th, int* tw) {
    const int in = r == 1 ? 16 : (r == 4 && elemSize == 1 ? 4 : 8);
    *th = kChromaRows * kChromaWaves;
    *tw = 64 * (in / elemSize / c);
}

} // namespace snnhip
