// espcn_f16_wide_a_body.h -- the body of kernel A16 wide (espcn_f16_wide.hip), #included by its kernels: espcn_f16_wide_conv_pair_kernel<K1, C1, C2,
// TIn, SIMPLE> (TIn = _Float16, or unsigned char: the 8-bit frame normalised while the tile is staged) and the 16-bit frame form
// espcn_f16_wide_conv_pair_u16_kernel (TIn = unsigned short), which carries a parameter block of its own -- textual inclusion as espcn_f16_a_body.h.
// In scope: K1, C1, C2, SIMPLE, the type TIn, the kernel arguments p, qin16 (a constant dummy in the kernels without a 16-bit frame), x, w1, w2, ep1,
// ep2, y.
    constexpr int TW = kEspcnF16WideTW_A, TH = kEspcnF16WideTH_A, P1 = K1 / 2;
    constexpr int C1W = TW + 2, C1H = TH + 2;                   // conv1 output region needed by conv2 (halo 1)
    constexpr int INW = C1W + 2 * P1, INH = C1H + 2 * P1;       // input region needed by conv1 on that region
    constexpr int NG1 = (C1H * C1W + 15) / 16;                  // 16-pixel groups of phase 1
    constexpr int GPR = TW / 16, RPW = TH / 4, G = GPR * RPW;   // phase 2: groups per row, rows per wave, groups per wave
    constexpr int MB1 = C1 / 16, MB2 = C2 / 16, KS2 = 9 * C1 / 32; // row blocks of conv1 / conv2, K-steps of conv2
    constexpr int U = 2;                                        // phase 1: groups in flight per wave
    static_assert(K1 * K1 <= 32, "conv1 is one K-step of 32 taps");
    static_assert(TW % 16 == 0 && TH % 4 == 0, "whole 16-pixel groups, whole rows per wave");
    static_assert(C1 % 32 == 0 && C2 % 16 == 0, "a K-step of conv2 is one tap and 32 channels; whole row blocks");
    static_assert((C1H * C1W * C1 + INH * INW) * 2 <= 65536, "static LDS");
    __shared__ __attribute__((aligned(16))) _Float16 s_c1[C1H * C1W * C1];
    __shared__ _Float16 s_in[INH * INW];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int px = lane & 15, g = lane >> 4;
    int b = xcd_tile_order(blockIdx.x, gridDim.x);
    const int tx = b % p.tilesX;
    b /= p.tilesX;
    const int ty = b % p.tilesY;
    const int n = b / p.tilesY;
    const int x0 = tx * TW, y0 = ty * TH;
    const TIn* xn = x + static_cast<size_t>(n) * p.H * p.W;

    // ---- phase 0 (A16's): input tile (origin y0-1-P1, x0-1-P1) -> LDS as halfs, zero outside the image
    {
        constexpr int NLD = (INH * INW + 255) / 256;
        _Float16 v[NLD];
#pragma unroll
        for (int k = 0; k < NLD; ++k) { // all loads in flight before the first LDS write
            const int idx = tid + k * 256;
            const int r = idx / INW, c = idx - r * INW;
            const int gy = y0 - 1 - P1 + r, gx = x0 - 1 - P1 + c;
            v[k] = static_cast<_Float16>(0.0f);
            if (idx < INH * INW && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) {
                const TIn u = xn[static_cast<size_t>(gy) * p.W + gx];
                if constexpr (FrameBits<TIn>::value == 16)
                    v[k] = static_cast<_Float16>((static_cast<float>(static_cast<unsigned>(u) >> qin16.shift) - qin16.mean) * qin16.norm);
                else if constexpr (FrameBits<TIn>::value == 8)
                    v[k] = static_cast<_Float16>((static_cast<float>(u) - p.mean) * p.norm);
                else
                    v[k] = static_cast<_Float16>(u);
            }
        }
#pragma unroll
        for (int k = 0; k < NLD; ++k)
            if (tid + k * 256 < INH * INW) s_in[tid + k * 256] = v[k];
    }

    // conv1's K axis = its taps: lane group g supplies taps 8g .. 8g+7 (a tap past the last one carries a zero weight and a zero value)
    int off1[8];
    bool tapok[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int t = 8 * g + j;
        tapok[j] = t < K1 * K1;
        const int tt = tapok[j] ? t : 0;
        off1[j] = (tt / K1) * INW + (tt % K1);
    }
    __syncthreads();

    // ---- phase 1: conv1 over the C1H x C1W halo region, pixels flattened into 16-wide groups: MB1 MFMAs per group on one B operand
    {
        f16x8 a1[MB1];
        float sc1[MB1][4], sh1[MB1][4];
#pragma unroll
        for (int mb = 0; mb < MB1; ++mb) {
            a1[mb] = *reinterpret_cast<const f16x8*>(w1 + (mb * 64 + lane) * 8);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sc1[mb][r] = ep1[(16 * mb + 4 * g + r) * 2];
                sh1[mb][r] = ep1[(16 * mb + 4 * g + r) * 2 + 1];
            }
        }
        for (int grp0 = wv * U; grp0 < NG1; grp0 += 4 * U) {
            f32x4 acc[U][MB1];
            int rr[U], cc[U];
            bool valid[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int pi = (grp0 + u) * 16 + px;
                valid[u] = pi < C1H * C1W;
                const int pc = valid[u] ? pi : C1H * C1W - 1;
                rr[u] = pc / C1W;
                cc[u] = pc - rr[u] * C1W;
                const _Float16* src = s_in + rr[u] * INW + cc[u];
                f16x8 bv;
#pragma unroll
                for (int j = 0; j < 8; ++j) bv[j] = tapok[j] ? src[off1[j]] : static_cast<_Float16>(0.0f);
#pragma unroll
                for (int mb = 0; mb < MB1; ++mb) acc[u][mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[mb], bv, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int gy = y0 - 1 + rr[u], gx = x0 - 1 + cc[u];
                const bool inside = gy >= 0 && gy < p.H && gx >= 0 && gx < p.W; // outside the image: conv2's zero padding
                _Float16* dst = s_c1 + (rr[u] * C1W + cc[u]) * C1 + (g & 1) * 4;
#pragma unroll
                for (int mb = 0; mb < MB1; ++mb) { // rows 16mb + 4g .. + 3 = the half (g & 1) of slot 2mb + (g >> 1)
                    f16x4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        o[r] = static_cast<_Float16>(inside ? apply_act<SIMPLE>(p.act1, fmaf(acc[u][mb][r], sc1[mb][r], sh1[mb][r]), 0.0f) : 0.0f);
                    if (valid[u]) *reinterpret_cast<f16x4*>(dst + wide_slot<C1>(2 * mb + (g >> 1), cc[u]) * 8) = o;
                }
            }
        }
    }
    // conv2's A operand and epilogue -> registers (the loads fly while the block gathers at the barrier)
    f16x8 a2[KS2][MB2];
#pragma unroll
    for (int ks = 0; ks < KS2; ++ks)
#pragma unroll
        for (int mb = 0; mb < MB2; ++mb) a2[ks][mb] = *reinterpret_cast<const f16x8*>(w2 + ((ks * MB2 + mb) * 64 + lane) * 8);
    float sc2[MB2][4], sh2[MB2][4];
#pragma unroll
    for (int mb = 0; mb < MB2; ++mb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sc2[mb][r] = ep2[(16 * mb + 4 * g + r) * 2];
            sh2[mb][r] = ep2[(16 * mb + 4 * g + r) * 2 + 1];
        }
    __syncthreads();

    // ---- phase 2: conv2, G x MB2 accumulators per wave
    f32x4 acc2[G][MB2];
#pragma unroll
    for (int gi = 0; gi < G; ++gi)
#pragma unroll
        for (int mb = 0; mb < MB2; ++mb) acc2[gi][mb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    conv3x3_wide_tile<C1, MB2, G, GPR, C1W>(s_c1, wv * RPW, px, g, a2, acc2);

    // ---- epilogue: lane holds output channels 16mb + 4g .. + 3 of pixel (row, col0 + px): 8-byte stores
    _Float16* yn = y + static_cast<size_t>(n) * p.H * p.W * C2;
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
        const int gy = y0 + wv * RPW + gi / GPR, gx = x0 + (gi % GPR) * 16 + px;
        if (gy < p.H && gx < p.W) {
#pragma unroll
            for (int mb = 0; mb < MB2; ++mb) {
                f16x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = static_cast<_Float16>(apply_act<SIMPLE>(p.act2, fmaf(acc2[gi][mb][r], sc2[mb][r], sh2[mb][r]), 0.0f));
                *reinterpret_cast<f16x4*>(yn + (static_cast<size_t>(gy) * p.W + gx) * C2 + 16 * mb + g * 4) = o;
            }
        }
    }
