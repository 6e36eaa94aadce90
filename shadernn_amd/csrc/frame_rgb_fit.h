// frame_rgb_fit.h -- what the fitted-RGB kernel of frame_rgb_fit.hip shares between its kernel, its plan and the tap table (include/snnhip.h:
// snnhip_rgb_fit_plan_create / snnhip_rgb_fit_taps): the four-tap table of one enlarging axis and the geometry of one
// (element size, source) instance.  The Keys cubic, the sample-format check and the quantiser are frame_resample.h's, the LDS budget, the block
// size and the row skew frame_fit.h's, the matrix coefficients frame_yuv_rgb.h's and the luma of a pixel frame_colour.h's.
#pragma once
#include "frame_colour.h"
#include "frame_fit.h"
#include "frame_yuv_rgb.h"

namespace snnhip {

constexpr int kRgbFitTaps = 4; // weights per output coordinate: taps at base - 1 .. base + 2

// The table of one axis with `in` source samples and `out` outputs, 1 <= out / in <= 8: row X holds the four weights of output X and base[X].
// The output is always a luma grid: output X reads source position s = (X + 1/2) in / out - off, off = 1/2 for aligned centres and 1/4 for a
// left-sited 4:2:0 chroma axis (sample i at luma column 2i).  In integers: a = 4 off, Nn = (4X + 2) in - a out, D = 4 out, base = floor(Nn / D),
// t = (Nn - base D) / D.  The weights are fill_fit_taps' with f = 1 -- eight Keys values at |k - 3 - t| summed in ascending order in double, each
// divided by the sum and rounded to float -- of which the outer four are exactly 0 (their distance is at least 2): the table keeps k = 2 .. 5.
inline int fill_rgb_fit_taps(const char* name, int in, int out, int siting, float* weights, int* base, int capacity) {
#pragma clang fp contract(off)
    SNNHIP_REQUIRE(weights && base, "%s: null argument", name);
    SNNHIP_REQUIRE(in >= 1 && out >= 1, "%s: %d -> %d samples (both at least 1)", name, in, out);
    SNNHIP_REQUIRE(siting_ok(siting), "%s: siting %d (SNNHIP_SITING_CENTRE or SNNHIP_SITING_LEFT)", name, siting);
    SNNHIP_REQUIRE(out >= in && out <= 8ll * in, "%s: %d -> %d samples is a ratio outside [1, 8]", name, in, out);
    SNNHIP_REQUIRE(static_cast<long long>(capacity) >= static_cast<long long>(kRgbFitTaps) * out, "%s: room for %d floats, %lld needed", name, capacity,
                   static_cast<long long>(kRgbFitTaps) * out);
    const long long a = siting == SNNHIP_SITING_LEFT ? 1 : 2;
    const long long D = 4ll * out;
    for (int X = 0; X < out; ++X) {
        const long long Nn = (4ll * X + 2) * in - a * out;
        long long b = Nn / D;
        if (Nn % D < 0) --b; // floor
        const double t = static_cast<double>(Nn - b * D) / static_cast<double>(D);
        double w[kFitTaps], sum = 0.0;
        for (int k = 0; k < kFitTaps; ++k) {
            w[k] = keys_cubic(std::fabs(static_cast<double>(k - 3) - t));
            sum += w[k];
        }
        base[X] = static_cast<int>(b);
        for (int k = 0; k < kRgbFitTaps; ++k) weights[static_cast<size_t>(kRgbFitTaps) * X + k] = static_cast<float>(w[k + 2] / sum);
    }
    return SNNHIP_OK;
}

// ---- geometry.  A block of kFitThreads threads owns an output tile of TH x TW pixels.  TW is one dword of the fitted luma row per lane of a wave
// (256 pixels of 8 bits, 128 of 16) and TH what the 48 KB of LDS hold of vertically filtered rows over the tile's source column span, two floats
// per source pixel.  The source is never shrunk: base advances by at most TW - 1 + 1 across a tile and four taps reach one pixel in front of it
// and two behind, TW + 4 pixels; the span is cut into strips of SP source pixels (what one lane loads of a row) and may start anywhere inside its
// first strip.
struct RgbFitGeom {
    int elemSize, source;
    constexpr int npx() const { return 4 / elemSize; }  // output pixels per lane and row: one dword of Yfit
    constexpr int tw() const { return 64 * npx(); }
    // source pixels of a strip: the CbCr pixels of one dword; one dword of each plane; four RGB(A) pixels (3 or 4 dwords)
    constexpr int sp() const { return source == SNNHIP_RGB_FIT_CBCR ? (elemSize == 1 ? 2 : 1) : source == SNNHIP_RGB_FIT_PLANAR ? 4 / elemSize : 4; }
    constexpr int spanPixels() const { return tw() + 4; }
    constexpr int maxStrips() const { return (spanPixels() + 2 * (sp() - 1)) / sp(); }
    constexpr int rowStride() const { return fit_skew(2 * maxStrips() * sp() - 1) + 1; } // floats
    constexpr int th() const { return kFitLdsFloats / rowStride() < kFitMaxRows ? kFitLdsFloats / rowStride() : kFitMaxRows; }
};

} // namespace snnhip
