// conv2d_mfma_pool_f16.hip -- the pooling (Conv2D -> MaxPooling2D 2x2 stride 2, chain rule L) f16 instances of conv2d_mfma_kernel, the three block
// widths with the wave layouts of conv2d_mfma_bn{128,64,32}_f16.hip; the kernel template and the variant table are in conv2d_mfma_kernel.h, the plan
// builder in conv2d_mfma.hip.
#include "conv2d_mfma_kernel.h"

namespace snnhip {

mfma_detail::PoolKernelFn pick_conv2d_mfma_pool_f16(int bn, int c8, int r, int taps) {
    if (bn == 128) return mfma_detail::pick_kernel_pool<2, 2, 2, 2, true>(c8, r, taps);
    if (bn == 64) return mfma_detail::pick_kernel_pool<2, 2, 2, 1, true>(c8, r, taps);
    return mfma_detail::pick_kernel_pool<4, 1, 1, 1, true>(c8, r, taps);
}

} // namespace snnhip
