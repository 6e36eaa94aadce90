// frame_colour.h -- what the two colour-frame kernels of frame_colour.hip share (include/snnhip.h: snnhip_rgb_luma_plan_create /
// snnhip_ycc_merge_plan_create): the luma of a pixel, the element types and the merge kernel's tile.  The Keys cubic, the aligned-centre phase
// (bicubic_phase), the quantiser and the check of kr / kb are frame_resample.h's.
#pragma once
#include "frame_resample.h"

namespace snnhip {

// low-resolution tile of one block of the merge kernel (every upscale factor)
constexpr int kMergeTileH = 8;
constexpr int kMergeTileW = 64;

// Full-range luma in fp32, unquantised: the luma plan rounds it, the merge kernel subtracts it from R and B.  Both call this one function.
__device__ __forceinline__ float luma_f32(float r, float g, float b, float kr, float kg, float kb) { return kr * r + kg * g + kb * b; }

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

} // namespace snnhip
