// espcn_f16_wide_b_body.h -- the body of kernel B16 wide<R> (espcn_f16_wide.hip), #included by its kernels: espcn_f16_wide_d2s_kernel<R, C2, TOut,
// SIMPLE> (TOut = _Float16 or unsigned char) and the 16-bit frame form espcn_f16_wide_d2s_u16_kernel (TOut = unsigned short).  Textual inclusion as
// espcn_f16_b_body.h; the store side is that kernel's (espcn_f16_d2s_store.h).
// In scope: R, C2, SIMPLE, the type TOut, the kernel arguments p, qout16 (a constant dummy in the kernels without a 16-bit frame), x, w, ep, y.
    constexpr int TW = kEspcnF16WideTW_B, TH = kEspcnF16WideTH_B, TWH = TW + 2, THH = TH + 2;
    constexpr int SL = C2 / 8;                                   // 16-byte slots per pixel
    constexpr int NCH = THH * TWH * SL, NLD = (NCH + 255) / 256; // 16-byte chunks of the halo tile; per thread
    constexpr int G = 4, KS = 9 * C2 / 32;                       // 16-pixel groups per wave: rows 2wv, 2wv+1 x column halves; K-steps
    static_assert(TW == 32 && TH == 8, "a wave owns 2 rows of 32 pixels = four 16-pixel groups");
    static_assert(R >= 2 && R <= 4, "rows 4*dy + dx: R <= 4");
    static_assert(C2 % 32 == 0, "a K-step is one tap and 32 channels");
    __shared__ __attribute__((aligned(16))) _Float16 s_x[THH * TWH * C2];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int px = lane & 15, g = lane >> 4;
    int b = xcd_tile_order(blockIdx.x, gridDim.x);
    const int tx = b % p.tilesX;
    b /= p.tilesX;
    const int ty = b % p.tilesY;
    const int n = b / p.tilesY;
    const int x0 = tx * TW, y0 = ty * TH;
    const _Float16* xn = x + static_cast<size_t>(n) * p.H * p.W * C2;

    // ---- halo tile (origin y0-1, x0-1) -> LDS, zero outside the image (the convolution's padding)
    {
        uint4 v[NLD];
#pragma unroll
        for (int k = 0; k < NLD; ++k) { // every load is in flight before the first LDS write
            const int idx = tid + k * 256;
            const int h = idx % SL, pix = idx / SL;
            const int r = pix / TWH, c = pix - r * TWH;
            const int gy = y0 - 1 + r, gx = x0 - 1 + c;
            v[k] = make_uint4(0u, 0u, 0u, 0u);
            if (idx < NCH && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W)
                v[k] = *reinterpret_cast<const uint4*>(xn + (static_cast<size_t>(gy) * p.W + gx) * C2 + h * 8);
        }
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int idx = tid + k * 256;
            const int h = idx % SL, pix = idx / SL;
            const int c = pix % TWH;
            if (idx < NCH) *reinterpret_cast<uint4*>(s_x + pix * C2 + wide_slot<C2>(h, c) * 8) = v[k];
        }
    }
    f16x8 a[KS][1];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) a[ks][0] = *reinterpret_cast<const f16x8*>(w + (ks * 64 + lane) * 8);
    float sc[4], sh[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sc[r] = ep[(4 * g + r) * 2];
        sh[r] = ep[(4 * g + r) * 2 + 1];
    }
    __syncthreads();

    f32x4 accw[G][1];
#pragma unroll
    for (int gi = 0; gi < G; ++gi) accw[gi][0] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    conv3x3_wide_tile<C2, 1, G, 2, TWH>(s_x, wv * 2, px, g, a, accw);
    f32x4 acc[G];
#pragma unroll
    for (int gi = 0; gi < G; ++gi) acc[gi] = accw[gi][0];

#include "espcn_f16_d2s_store.h"
