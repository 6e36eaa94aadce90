// frame_tensor_yuv.h -- what the output-tensor -> video-frame kernel of frame_tensor_yuv.hip shares between its kernel, its plan and the coefficient
// table (include/snnhip.h: snnhip_tensor_yuv_plan_create / snnhip_tensor_yuv_planar_plan_create / snnhip_tensor_yuv_coefficients; DESIGN.md section
// 4.27): the five coefficients and the lane geometry.  The luma of a pixel is frame_colour.h's, the one function rgb_luma, ycc_merge and rgb_cbcr
// call; the quantiser, the sample-format checks and the dword stores are frame_resample.h's; the ranges are frame_yuv_rgb.h's.
#pragma once
#include "frame_colour.h"
#include "frame_yuv_rgb.h"

namespace snnhip {

// Full-range RGB at `maxval` -> Y'CbCr codes: the inverse of yuv_rgb's matrix, computed in double and rounded to float.  ys = 1 / cy, cbs = 1 / cbu
// and crs = 1 / crv of yuv_rgb_coeffs, each formed from the ranges themselves and not by dividing the rounded floats.
struct TensorYuvCoeffs {
    float yoff, ys, coff, cbs, crs; // yoff, coff exact: multiples of (maxval + 1) / 256
};
inline TensorYuvCoeffs tensor_yuv_coeffs(int maxval, int range, double kr, double kb) {
#pragma clang fp contract(off)
    const double k = (maxval + 1) / 256.0, m = maxval;
    const bool limited = range == SNNHIP_RANGE_LIMITED;
    const double yoff = limited ? 16.0 * k : 0.0, yrange = limited ? 219.0 * k : m, crange = limited ? 224.0 * k : m;
    TensorYuvCoeffs c;
    c.yoff = static_cast<float>(yoff);
    c.ys = static_cast<float>(yrange / m);
    c.coff = static_cast<float>(128.0 * k);
    c.cbs = static_cast<float>(crange / (2.0 * (1.0 - kb) * m));
    c.crs = static_cast<float>(crange / (2.0 * (1.0 - kr) * m));
    return c;
}

constexpr int kTensorYuvThreads = 256;

// A lane owns a strip of two luma rows and S columns, and the S / 2 chroma samples under it.  S is the fewest columns at which every run the lane
// stores -- a luma row, a row of one chroma plane, a row of the interleaved plane -- is whole dwords: 4 bytes of one PLANAR chroma plane are 8 luma
// columns of 8-bit samples and 4 of 16-bit ones; 4 bytes of the INTERLEAVED plane are two 8-bit CbCr pairs (4 columns) or one 16-bit pair (2).
constexpr int tensor_yuv_strip(int elemSize, bool planar) { return (planar ? 8 : 4) / elemSize; }
// luma pixels of one block: the tile snnhip_plan_describe reports
constexpr int tensor_yuv_tile(int elemSize, bool planar) { return kTensorYuvThreads * 2 * tensor_yuv_strip(elemSize, planar); }

} // namespace snnhip
