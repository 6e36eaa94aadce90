// espcn_d2s_mfma.hip -- chain rule B for upscale factors R = 3 and 4: conv 3x3 (16 -> R*R) + act -> depth-to-space(R) + tanh on the fp32 matrix
// cores (v_mfma_f32_16x16x4_f32), and its 8-bit form (rule B8).  One body for both kernels, espcn_d2s_mfma_body.h; the rule itself (pattern match,
// weight image, cost) is in the chain planner, chain_fuse.hip.  R = 2 keeps its own kernels in espcn_fused.hip.  DESIGN.md section 4.10.
#include <hip/hip_ext.h>

#include "espcn_common.h"
#include "espcn_d2s_mfma.h"
#include "snnhip_internal.h"

namespace snnhip {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int R, bool SIMPLE>
__global__ __launch_bounds__(256, 4) void conv3x3_c16oR_d2s_tanh_kernel(EspcnD2sParams p, const float* __restrict__ x, const float* __restrict__ w,
                                                                        const float* __restrict__ ep, float* __restrict__ y) {
    typedef float TOut;
    constexpr U8OutCfg qout{0.0f, 0.0f};
    constexpr U16OutCfg qout16{0.0f, 0.0f, 0.0f, 0};
#include "espcn_d2s_mfma_body.h"
}

template <int R, bool SIMPLE>
__global__ __launch_bounds__(256, 4) void conv3x3_c16oR_d2s_tanh_u8_kernel(EspcnD2sParams p, U8OutCfg qout, const float* __restrict__ x,
                                                                           const float* __restrict__ w, const float* __restrict__ ep,
                                                                           unsigned char* __restrict__ y) {
    typedef unsigned char TOut;
    constexpr U16OutCfg qout16{0.0f, 0.0f, 0.0f, 0};
#include "espcn_d2s_mfma_body.h"
}

// the 16-bit form (snnhip_u16_out_plan_create folded in)
template <int R, bool SIMPLE>
__global__ __launch_bounds__(256, 4) void conv3x3_c16oR_d2s_tanh_u16_kernel(EspcnD2sParams p, U16OutCfg qout16, const float* __restrict__ x,
                                                                            const float* __restrict__ w, const float* __restrict__ ep,
                                                                            unsigned short* __restrict__ y) {
    typedef unsigned short TOut;
    constexpr U8OutCfg qout{0.0f, 0.0f};
#include "espcn_d2s_mfma_body.h"
}

template <int R, bool S>
int launch_br(hipStream_t stream, dim3 grid, const EspcnD2sParams& p, const FrameOut& f, const float* x, const float* w, const float* ep, void* y,
               hipEvent_t evStart, hipEvent_t evStop) {
    if (f.bits == 16)
        SNNHIP_LAUNCH_EV((conv3x3_c16oR_d2s_tanh_u16_kernel<R, S>), grid, dim3(256), 0, stream, evStart, evStop, p, U16OutCfg{f.scale, f.offset, f.maxval, f.shift},
                         x, w, ep, static_cast<unsigned short*>(y));
    else if (f.bits == 8)
        SNNHIP_LAUNCH_EV((conv3x3_c16oR_d2s_tanh_u8_kernel<R, S>), grid, dim3(256), 0, stream, evStart, evStop, p, U8OutCfg{f.scale, f.offset}, x, w, ep,
                         static_cast<unsigned char*>(y));
    else
        SNNHIP_LAUNCH_EV((conv3x3_c16oR_d2s_tanh_kernel<R, S>), grid, dim3(256), 0, stream, evStart, evStop, p, x, w, ep, static_cast<float*>(y));
    SNNHIP_CHECK_HIP(hipGetLastError());
    return SNNHIP_OK;
}

} // namespace

int espcn_d2s_mfma_launch(hipStream_t stream, int r, const EspcnD2sParams& p, const FrameOut& f, const float* x, const float* w, const float* ep, void* y,
                          hipEvent_t evStart, hipEvent_t evStop) {
    SNNHIP_REQUIRE(r == 3 || r == 4, "espcn_d2s_mfma: upscale factor %d (3 or 4)", r);
    const dim3 grid(p.tilesX * p.tilesY * p.N);
    const bool simple = act_is_simple(p.act.act);
    if (r == 3)
        return simple ? launch_br<3, true>(stream, grid, p, f, x, w, ep, y, evStart, evStop) : launch_br<3, false>(stream, grid, p, f, x, w, ep, y, evStart, evStop);
    return simple ? launch_br<4, true>(stream, grid, p, f, x, w, ep, y, evStart, evStop) : launch_br<4, false>(stream, grid, p, f, x, w, ep, y, evStart, evStop);
}

} // namespace snnhip
