// frame_yuv_tensor.h -- what the video-frame -> input-tensor kernel of frame_yuv_tensor.hip shares between its kernel, its plan and the tap table
// (include/snnhip.h: snnhip_yuv_tensor_plan_create / snnhip_yuv_tensor_planar_plan_create / snnhip_yuv_tensor_taps): the lane
// geometry and one coordinate of a sampling table.  The matrix, the 4:2:0 tap table, the Keys cubic, the sample-format checks and frame_elem are
// frame_yuv_rgb.h's and frame_resample.h's.
#pragma once
#include "frame_yuv_rgb.h"

namespace snnhip {

constexpr int kYuvTensorThreads = 256;

// The output [N][OH][OW][C] is one flat run of N * OH * OW pixels; a lane owns LP consecutive ones, so that what it stores is whole dwords that start
// on a dword: one fp32 pixel (C dwords), one RGBA fp16 pixel (2 dwords), or TWO RGB fp16 pixels (6 + 6 bytes = 3 dwords: a single one is 6 bytes and
// every other one starts 2 bytes off a dword).  A pair may straddle the end of a row or of an image; the two pixels are independent.
constexpr int yuv_tensor_lane_pixels(int C, bool half) { return half && C == 3 ? 2 : 1; }
// flat output pixels of one block: the tile snnhip_plan_describe reports
constexpr int yuv_tensor_tile(int C, bool half) { return kYuvTensorThreads * yuv_tensor_lane_pixels(C, half); }

// one output coordinate of an axis: the two source indices, clamped to the plane, and the weight of the second (nearest: i1 = i0, a = 0)
struct YuvTensorCoord {
    int i0, i1;
    float a;
    int pad;
};

} // namespace snnhip
