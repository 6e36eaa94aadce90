// frame_rgb_fit.h -- what the fitted-RGB kernel of frame_rgb_fit.hip adds to the fit core (frame_fit_core.h; include/snnhip.h:
// snnhip_rgb_fit_plan_create / snnhip_rgb_fit_taps): its rule for the four-tap table of one enlarging axis and the strips of
// one (element size, source) instance.  The matrix coefficients are frame_yuv_rgb.h's and the luma of a pixel frame_colour.h's.
#pragma once
#include "frame_colour.h"
#include "frame_fit_core.h"
#include "frame_yuv_rgb.h"

namespace snnhip {

constexpr int kRgbFitTaps = 4; // weights per output coordinate: taps at base - 1 .. base + 2

// The table of one axis with `in` source samples and `out` outputs, 1 <= out / in <= 8.  The output is always a luma grid: output X reads source
// position s = (X + 1/2) in / out - off, off = 1/2 for aligned centres and 1/4 for a left-sited 4:2:0 chroma axis (sample i at luma column 2i).
// Never shrinking, f = 1 and the outer four of the eight weights are exactly 0 (their distance is at least 2): the table keeps k = 2 .. 5.
constexpr FitRule kRgbFitRule{false, false, 1, 8, "[1, 8]", 2, kRgbFitTaps};

// ---- geometry.  TW is one dword of the fitted luma row per lane of a wave (256 pixels of 8 bits, 128 of 16), a filtered row has two floats per
// source pixel.  The source is never shrunk: base advances by at most TW - 1 + 1 across a tile and four taps reach one pixel in front of it and two
// behind, TW + 4 pixels; the span is cut into strips of SP source pixels and may start anywhere inside its first strip.
struct RgbFitGeom {
    int elemSize, source;
    constexpr int npx() const { return 4 / elemSize; }  // output pixels per lane and row: one dword of Yfit
    constexpr int tw() const { return 64 * npx(); }
    // source pixels of a strip: the CbCr pixels of one dword; one dword of each plane; four RGB(A) pixels (3 or 4 dwords)
    constexpr int sp() const { return source == SNNHIP_RGB_FIT_CBCR ? (elemSize == 1 ? 2 : 1) : source == SNNHIP_RGB_FIT_PLANAR ? 4 / elemSize : 4; }
    constexpr int spanPixels() const { return tw() + 4; }
    constexpr int maxStrips() const { return (spanPixels() + 2 * (sp() - 1)) / sp(); }
    constexpr FitTile tile() const { return FitTile{tw(), 2 * sp(), maxStrips()}; }
    // the span of a tile whose first and last columns have bases b0 and b1: pixels px0 = first(b0), a multiple of SP at or below its first pixel, .. b1 + 2
    constexpr int first(int b0) const { return (b0 - 1) & ~(sp() - 1); } // (two's complement: the floor for the columns left of the source)
    constexpr int strips(int px0, int b1) const { return (b1 + 2 - px0) / sp() + 1; }
};

} // namespace snnhip
