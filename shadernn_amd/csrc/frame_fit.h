// frame_fit.h -- what the general-ratio plane resampler of frame_fit.hip adds to the fit core (frame_fit_core.h; include/snnhip.h:
// snnhip_plane_fit_plan_create / snnhip_fit_taps): its rule for the table of one axis and the strips of one (E, C, WIDE) instance.
#pragma once
#include "frame_fit_core.h"

namespace snnhip {

// The table of one axis with `in` inputs and `out` outputs, 1/2 <= out / in <= 4.  Output X reads source position s = (X + lead) * in / out - lead,
// lead = siting_offset(siting): the output grid is sited as the input is.  All eight weights are kept; the kernel is stretched when shrinking.
constexpr FitRule kPlaneFitRule{true, true, 2, 4, "[1/2, 4]", 0, kFitTaps};

// ---- geometry.  TW is 256 bytes of an output row and a strip one dword of an input row.  WIDE instances serve plans with a shrinking axis (all
// eight taps live, the span up to 2 TW + 8 pixels); the others read the inner four taps only (the outer four are exactly 0 when enlarging) and span
// at most TW + 5 pixels.
struct FitGeom {
    int elemSize, C, wide;
    constexpr int ne() const { return 4 / elemSize; }                  // elements per dword
    constexpr int tw() const { return 256 / (C * elemSize); }          // tile width in output pixels
    constexpr int k0() const { return wide ? 0 : 2; }                  // first tap read
    constexpr int taps() const { return wide ? 8 : 4; }                // taps read
    constexpr int lo() const { return 3 - k0(); }                      // pixels in front of base
    constexpr int hi() const { return k0() + taps() - 4; }             // pixels behind base
    // input pixels under a full tile at most: base advances by at most (TW - 1) * (2 or 1) + 1 across it
    constexpr int spanPixels() const { return (tw() - 1) * (wide ? 2 : 1) + 2 + lo() + hi(); }
    // ... as dword strips of a row: the span may start anywhere inside its first dword
    constexpr int maxStrips() const { return (spanPixels() * C + ne() - 1 + ne() - 1) / ne(); }
    constexpr FitTile tile() const { return FitTile{tw(), ne(), maxStrips()}; }
    // the span of a tile whose first and last columns have bases b0 and b1: from element e0 = first(b0), a multiple of NE at or below its first element
    constexpr int first(int b0) const { return ((b0 - lo()) * C) & ~(ne() - 1); }
    constexpr int strips(int e0, int b1) const {
        const int eLast = (b1 + hi()) * C + C - 1;
        return (eLast - e0) / ne() + 1;
    }
};

} // namespace snnhip
