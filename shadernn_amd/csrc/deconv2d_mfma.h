// deconv2d_mfma.h -- Conv2DTranspose on the matrix cores (deconv2d_mfma.hip): what snnhip_deconv2d_plan_create (shape_ops.hip) needs of it.
#pragma once
#include "snnhip_internal.h"

namespace snnhip {

// The resolved layer of include/snnhip.h's transposed-convolution contract: square kernel k, stride s, p = padT, output extent from the caller.
struct DeconvGeom {
    int N, H, W, IC, OC, k, s, p, OH, OW, act, useBN;
    float leaky;
};

// s <= 4, ceil(k / s) <= 5, IC >= 16 and OC >= 16, the extent within s*H + k - s, and the kernel's own limits (halo tile within 64 KB of LDS, grid and
// weight image within its 32-bit indices).  Everything else stays on deconv2d_direct.
bool deconv2d_mfma_eligible(const DeconvGeom& g);

// epi4: make_epilogue_table(OC, 64, ...).  The plan adapts to fp32 or fp16 tensors per run and names the kernel of the last run in its description.
int make_deconv2d_mfma_plan(snnhip_ctx* ctx, const DeconvGeom& g, const float* w_oihw, const std::vector<float>& epi4, snnhip_plan** out);

} // namespace snnhip
