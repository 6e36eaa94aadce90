// espcn_d2s_mfma.h -- chain rule B for upscale factors 3 and 4 (espcn_d2s_mfma.hip): what the chain planner (chain_fuse.hip) needs to launch it.
#pragma once
#include <hip/hip_runtime.h>

#include "epilogue.h"
#include "espcn_fused.h"

namespace snnhip {

constexpr int kD2sMfmaTW = 32, kD2sMfmaTH = 8; // low-resolution pixels per block

using EspcnD2sParams = FusedBParams; // input [N, H, W, 16]; tiles of kD2sMfmaTW x kD2sMfmaTH; same fields, same tile decode as kernel B for upscale 2

// Conv2D 3x3 (16 -> r*r) + act -> depth-to-space(r) + tanh in one launch, r = 3 or 4.  w: the lane-ordered A-operand image (36 x 64 floats, MFMA
// row 4*dy + dx = channel r*dy + dx), ep: 16 x {scale, shift} in MFMA row order.  f: what y takes -- floats, an 8-bit frame, q = quantize_u8(o,
// scale, offset), or a 16-bit one, q = quantize_u16(o, scale, offset, maxval) << shift.  evStart / evStop: a plan-profile event pair or null.
inline bool espcn_d2s_mfma_takes_frame() { return true; } // its one form writes frames
int espcn_d2s_mfma_launch(hipStream_t stream, int r, const EspcnD2sParams& p, const FrameOut& f, const float* x, const float* w, const float* ep, void* y,
                          hipEvent_t evStart, hipEvent_t evStop);

} // namespace snnhip
