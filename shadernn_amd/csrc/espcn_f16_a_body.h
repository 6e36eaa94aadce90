// espcn_f16_a_body.h -- the body of kernel A16 (espcn_f16.hip), #included by its kernels: espcn_f16_conv_pair_kernel<K1, TIn, SIMPLE> (TIn = _Float16,
// or unsigned char: the 8-bit frame normalised while the tile is staged, half((float(u) - p.mean) * p.norm)) and the 16-bit frame form
// espcn_f16_conv_pair_u16_kernel (TIn = unsigned short: half((float(u >> qin16.shift) - qin16.mean) * qin16.norm), snnhip_u16_in_plan_create's fp16
// map).  Textual inclusion for the reason espcn_wino_a_body.h gives: the 16-bit form carries a parameter block of its own and the existing kernels
// stay instruction for instruction what they were.  A 16-bit frame element and a half are both 2 bytes: the body asks FrameBits<TIn>, not sizeof.
// In scope: K1, SIMPLE, the type TIn, the kernel arguments p, qin16 (a constant dummy in the kernels without a 16-bit frame), x, w1, w2, ep1, ep2, y.
    constexpr int TW = kEspcnF16TW_A, TH = kEspcnF16TH_A, P1 = K1 / 2;
    constexpr int C1W = TW + 2, C1H = TH + 2;                   // conv1 output region needed by conv2 (halo 1)
    constexpr int INW = C1W + 2 * P1, INH = C1H + 2 * P1;       // input region needed by conv1 on that region
    constexpr int NG1 = (C1H * C1W + 15) / 16;                  // 16-pixel groups of phase 1
    constexpr int GPR = TW / 16, RPW = TH / 4, G = GPR * RPW;   // phase 2: groups per row, rows per wave, groups (= accumulators) per wave
    constexpr int U = 2;                                        // phase 1: groups in flight per wave
    static_assert(K1 * K1 <= 32, "conv1 is one K-step of 32 taps");
    static_assert(TW % 16 == 0 && TH % 4 == 0, "whole 16-pixel groups, whole rows per wave");
    __shared__ __attribute__((aligned(16))) _Float16 s_c1[C1H * C1W * 16];
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

    // ---- phase 0: input tile (origin y0-1-P1, x0-1-P1) -> LDS as halfs, zero outside the image
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

    // ---- weights -> registers (the host packed them in lane order), epilogue (scale, shift) of this lane's four rows
    const f16x8 a1 = *reinterpret_cast<const f16x8*>(w1 + lane * 8);
    const W3Regs a2 = load_w3(w2, lane);
    float sc1[4], sh1[4], sc2[4], sh2[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sc1[r] = ep1[(4 * g + r) * 2];
        sh1[r] = ep1[(4 * g + r) * 2 + 1];
        sc2[r] = ep2[(4 * g + r) * 2];
        sh2[r] = ep2[(4 * g + r) * 2 + 1];
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

    // ---- phase 1: conv1 over the C1H x C1W halo region, pixels flattened into 16-wide groups: one MFMA per group
    for (int grp0 = wv * U; grp0 < NG1; grp0 += 4 * U) {
        f32x4 acc[U];
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
            acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, bv, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int gy = y0 - 1 + rr[u], gx = x0 - 1 + cc[u];
            const bool inside = gy >= 0 && gy < p.H && gx >= 0 && gx < p.W; // outside the image: conv2's zero padding
            f16x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                o[r] = static_cast<_Float16>(inside ? apply_act<SIMPLE>(p.act1, fmaf(acc[u][r], sc1[r], sh1[r]), 0.0f) : 0.0f);
            if (valid[u]) *reinterpret_cast<f16x4*>(s_c1 + (rr[u] * C1W + cc[u]) * 16 + slot_off(g >> 1, cc[u]) + (g & 1) * 4) = o;
        }
    }
    __syncthreads();

    // ---- phase 2: conv2, G accumulators per wave
    f32x4 acc2[G];
#pragma unroll
    for (int gi = 0; gi < G; ++gi) acc2[gi] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    conv3x3_c16_tile<G, GPR, C1W>(s_c1, wv * RPW, px, g, a2, acc2);

    // ---- epilogue: lane holds output channels 4g .. 4g+3 of pixel (row, col0 + px): 8-byte stores
    _Float16* yn = y + static_cast<size_t>(n) * p.H * p.W * 16;
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
        const int gy = y0 + wv * RPW + gi / GPR, gx = x0 + (gi % GPR) * 16 + px;
        if (gy < p.H && gx < p.W) {
            f16x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = static_cast<_Float16>(apply_act<SIMPLE>(p.act2, fmaf(acc2[gi][r], sc2[r], sh2[r]), 0.0f));
            *reinterpret_cast<f16x4*>(yn + (static_cast<size_t>(gy) * p.W + gx) * 16 + g * 4) = o;
        }
    }
