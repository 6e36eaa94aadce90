// frame_fit.h -- what the general-ratio plane resampler of frame_fit.hip shares between its kernel, its plan and the tap table
// (include/snnhip.h: snnhip_plane_fit_plan_create / snnhip_fit_taps): the table of one axis and the geometry of one
// (E, C, WIDE) instance.  The Keys cubic, the siting offset, the sample-format check and the quantiser are frame_resample.h's.
#pragma once
#include "frame_resample.h"

namespace snnhip {

constexpr int kFitTaps = 8; // weights per output coordinate: taps at base - 3 .. base + 4

// The table of one axis with `in` inputs and `out` outputs, 1/2 <= out / in <= 4: row X holds the eight weights of output X and base[X].
// Output X reads source position s = (X + lead) * in / out - lead, lead = siting_offset(siting), in integers: a = 4 lead, Nn = (4X + a) in - a out,
// D = 4 out, base = floor(Nn / D), t = (Nn - base D) / D.  Tap k sits at base - 3 + k, its weight is the Keys cubic at |k - 3 - t| * f,
// f = min(out / in, 1) (the kernel stretched when shrinking); the eight are summed in ascending order in double, divided by the sum and rounded to float.
inline int fill_fit_taps(const char* name, int in, int out, int siting, float* weights, int* base, int capacity) {
#pragma clang fp contract(off)
    SNNHIP_REQUIRE(weights && base, "%s: null argument", name);
    SNNHIP_REQUIRE(in >= 1 && out >= 1, "%s: %d -> %d samples (both at least 1)", name, in, out);
    SNNHIP_REQUIRE(siting_ok(siting), "%s: siting %d (SNNHIP_SITING_CENTRE or SNNHIP_SITING_LEFT)", name, siting);
    SNNHIP_REQUIRE(2ll * out >= in && out <= 4ll * in, "%s: %d -> %d samples is a ratio outside [1/2, 4]", name, in, out);
    SNNHIP_REQUIRE(static_cast<long long>(capacity) >= static_cast<long long>(kFitTaps) * out, "%s: room for %d floats, %lld needed", name, capacity,
                   static_cast<long long>(kFitTaps) * out);
    const long long a = siting == SNNHIP_SITING_LEFT ? 1 : 2;
    const long long D = 4ll * out;
    const double f = out < in ? static_cast<double>(out) / static_cast<double>(in) : 1.0;
    for (int X = 0; X < out; ++X) {
        const long long Nn = (4ll * X + a) * in - a * out;
        long long b = Nn / D;
        if (Nn % D < 0) --b; // floor
        const double t = static_cast<double>(Nn - b * D) / static_cast<double>(D);
        double w[kFitTaps], sum = 0.0;
        for (int k = 0; k < kFitTaps; ++k) {
            w[k] = keys_cubic(std::fabs(static_cast<double>(k - 3) - t) * f);
            sum += w[k];
        }
        base[X] = static_cast<int>(b);
        for (int k = 0; k < kFitTaps; ++k) weights[static_cast<size_t>(kFitTaps) * X + k] = static_cast<float>(w[k] / sum);
    }
    return SNNHIP_OK;
}

// ---- geometry.  A block of 256 threads owns an output tile of TH x TW pixels.  TW is 256 bytes of an output row -- 64 dwords, one per lane of a
// wave -- and TH what the 48 KB of LDS hold of vertically filtered float rows over the tile's input column span.  WIDE instances serve plans with
// a shrinking axis (all eight taps live, the span up to 2 TW + 8 pixels); the others read the inner four taps only (the outer four are exactly 0
// when enlarging) and span at most TW + 5 pixels.
constexpr int kFitThreads = 256;
constexpr int kFitLdsFloats = 12288; // 48 KB of static LDS: three blocks per CU
constexpr int kFitMaxRows = 32;      // output rows per tile at most
// rows of floats are skewed by one float every 32: lanes that start 4 or 8 floats apart (a dword of outputs at ratio 1 or 1/2) then fall on 32
// different banks of a ds_read_b32 instead of 8 or 4
__host__ __device__ constexpr int fit_skew(int i) { return i + (i >> 5); }

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
    constexpr int rowStride() const { return fit_skew(maxStrips() * ne() - 1) + 1; } // floats
    constexpr int th() const { return kFitLdsFloats / rowStride() < kFitMaxRows ? kFitLdsFloats / rowStride() : kFitMaxRows; }
};

} // namespace snnhip
