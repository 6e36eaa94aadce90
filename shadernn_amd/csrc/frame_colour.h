// frame_colour.h -- the arithmetic shared by the two colour-frame kernels of frame_colour.hip (include/snnhip.h: snnhip_rgb_luma_plan_create /
// snnhip_ycc_merge_plan_create) and the host-side tap table (snnhip_bicubic_taps).  One definition each: the luma of a pixel, the quantiser and the
// Keys cubic.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace snnhip {

// low-resolution tile of one block of the merge kernel (every upscale factor)
constexpr int kMergeTileH = 8;
constexpr int kMergeTileW = 64;

// Full-range luma in fp32, unquantised: the luma plan rounds it, the merge kernel subtracts it from R and B.  Both call this one function.
__device__ __forceinline__ float luma_f32(float r, float g, float b, float kr, float kg, float kb) { return kr * r + kg * g + kb * b; }

// clamp(rint(v), 0, maxval), ties to even, NaN -> 0
__device__ __forceinline__ unsigned quantize_frame(float v, float maxval) {
    v = rintf(v);
    v = v >= 0.0f ? v : 0.0f; // NaN fails the test: 0
    v = v <= maxval ? v : maxval;
    return static_cast<unsigned>(v);
}

template <typename E>
struct FrameElem;
template <>
struct FrameElem<unsigned char> {
    static constexpr float maxval = 255.0f;
};
template <>
struct FrameElem<unsigned short> { // (16-bit colour frames are not shipped: the kernels are only written so that they can be instantiated)
    static constexpr float maxval = 65535.0f;
};

// Keys cubic convolution kernel, a = -0.5 (Catmull-Rom), at distance d >= 0; plain products in double, no contraction, so that the same expression in
// any IEEE double arithmetic gives the same bits
inline double keys_cubic(double d) {
#pragma clang fp contract(off)
    const double a = -0.5;
    if (d <= 1.0) return (a + 2.0) * (d * d * d) - (a + 3.0) * (d * d) + 1.0;
    if (d < 2.0) return a * (d * d * d) - 5.0 * a * (d * d) + 8.0 * a * d - 4.0 * a;
    return 0.0;
}

// Output sample X = r*x + p of an r-fold upscale with aligned pixel centres reads source position sx = (X + 0.5) / r - 0.5 = x + (p + 0.5) / r - 0.5:
// i0 = floor(sx) = x + first[p] (first[p] is -1 or 0), taps at i0 - 1 .. i0 + 2 with the Keys weights at distances 1 + t, t, 1 - t, 2 - t.
inline void bicubic_phase(int r, int p, int* first, double w[4]) {
#pragma clang fp contract(off)
    const double sx = (p + 0.5) / r - 0.5;
    const double i0 = std::floor(sx);
    const double t = sx - i0;
    *first = static_cast<int>(i0);
    w[0] = keys_cubic(1.0 + t);
    w[1] = keys_cubic(t);
    w[2] = keys_cubic(1.0 - t);
    w[3] = keys_cubic(2.0 - t);
}

} // namespace snnhip
