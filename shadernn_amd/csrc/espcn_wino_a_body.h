// espcn_wino_a_body.h -- the body of kernel A's Winograd form (espcn_fused.hip; the rules are chain_fuse.hip's), #included by its three kernels: rule A's (TIn = float), rule A8's
// (TIn = unsigned char: the 8-bit frame is normalised while the tile is staged, y = (float(u) - qin.mean) * qin.norm, snnhip_u8_in_plan_create's
// map; taps outside the image stay 0 in the NORMALISED domain, as the separate u8_in launch in front of rule A gives them) and the 16-bit form
// (TIn = unsigned short: y = (float(u >> qin16.shift) - qin16.mean) * qin16.norm, snnhip_u16_in_plan_create's map).  Textual inclusion
// rather than a shared __device__ function: inlining a body through a call changed the fp32 kernels' register allocation (scratch spills in
// <5,16,2,2>), and the fp32 instruction stream must stay what it was.  In scope: the template parameters K1, TH, AM, WPS, the type TIn, the
// kernel arguments p, qin, qin16 (each a constant dummy where the kernel has no such frame), x, wA1, wU, ep1, ep2, y.
    constexpr int kBits = FrameBits<TIn>::value;     // 0: fp32 input; 8 / 16: a frame, kept raw in the prefetch registers
    constexpr bool kFrame = kBits != 0;
    constexpr unsigned kOutside = kBits == 16 ? 65536u : 256u; // "outside the image": a value no load of the frame can produce
    constexpr int TW = WinoTile::TW, U = 2;
    constexpr int P1 = K1 / 2;
    constexpr int C1W = TW + 2, C1H = TH + 2;
    constexpr int C1P = 40, HALFP = 20;                        // LDS row pitch / odd-column plane offset, in pixels (see phase 2)
    constexpr int INW = TW + 2 + 2 * P1, INH = TH + 2 + 2 * P1;
    constexpr int INP = 48;                                    // LDS row pitch of the input tile: == 16 (mod 32) puts the four tap rows a
                                                               // wave reads in one ds_read_b32 (lane group g -> row g) on disjoint banks
    constexpr int KS1 = wino_conv1_ksteps(K1);
    constexpr int NG1 = (C1H * C1W + 15) / 16;                 // 16-pixel groups of phase 1
    constexpr int GPW = (NG1 + 3) / 4;                         // groups per wave (contiguous range)
    constexpr int NIT = (GPW + U - 1) / U;
    constexpr int GROUPS2 = TH / 8;                            // Winograd tile rows (= phase-2 groups) per wave
    constexpr int NLD = (INH * INP + 8 + 255) / 256;
    static_assert(INW <= INP, "input pitch");
    static_assert(C1W / 2 + 1 <= HALFP && HALFP + C1W / 2 <= C1P, "plane layout");

    __shared__ __attribute__((aligned(16))) float smem[C1H * C1P * 16 + 4096 + INH * INP + 8];
    float* s_c1 = smem;
    float* s_U = smem + C1H * C1P * 16;
    float* s_in = s_U + 4096;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int px = lane & 15, g = lane >> 4;
    const int ntiles = p.tilesX * p.tilesY * p.N;

    // Persistent blocks (grid = WPS per CU): weights / epilogue constants are loaded once per block and the input tile of the
    // NEXT tile is fetched into NLD registers while this tile is computed, so no wave ever waits on HBM inside the loop.
    auto tile_origin = [&](int t, int& n, int& x0, int& y0) {
        int b = xcd_tile_order(t, ntiles);
        const int tx = b % p.tilesX;
        b /= p.tilesX;
        const int ty = b % p.tilesY;
        n = b / p.tilesY;
        x0 = tx * TW;
        y0 = ty * TH;
    };
    float vin[NLD];
    unsigned vraw[kFrame ? NLD : 1]; // (frame input only)
    auto issue_loads = [&](int t) { // input tile (origin y0-1-P1, x0-1-P1), zero padded (+8 zero floats: invalid taps read them)
        int n, x0, y0;
        tile_origin(t, n, x0, y0);
        const TIn* xn = x + static_cast<size_t>(n) * p.H * p.W;
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int idx = tid + k * 256;
            const int r = idx / INP, c = idx - r * INP;
            const int gy = y0 - 1 - P1 + r, gx = x0 - 1 - P1 + c;
            if constexpr (kFrame) {
                // the raw byte straight into its register (no conversion here: that would wait for the load, and these loads are the prefetch of
                // the NEXT tile); kOutside = outside the image.  Normalised in store_input, after the tile's compute.
                vraw[k] = kOutside;
                if (r < INH && c < INW && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) vraw[k] = xn[static_cast<size_t>(gy) * p.W + gx];
            } else {
                vin[k] = 0.0f;
                if (r < INH && c < INW && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) vin[k] = xn[static_cast<size_t>(gy) * p.W + gx];
            }
        }
    };
    auto store_input = [&]() {
#pragma unroll
        for (int k = 0; k < NLD; ++k)
            if (tid + k * 256 < INH * INP + 8) {
                if constexpr (kBits == 16) s_in[tid + k * 256] = vraw[k] < kOutside ? (static_cast<float>(vraw[k] >> qin16.shift) - qin16.mean) * qin16.norm : 0.0f;
                else if constexpr (kFrame) s_in[tid + k * 256] = vraw[k] < kOutside ? (static_cast<float>(vraw[k]) - qin.mean) * qin.norm : 0.0f;
                else s_in[tid + k * 256] = vin[k];
            }
    };

    int tile = blockIdx.x;
    if (tile >= ntiles) return;
    SNNHIP_STAMP(0);
    issue_loads(tile);
    {
        float4 u[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) u[k] = reinterpret_cast<const float4*>(wU)[tid + k * 256];
#pragma unroll
        for (int k = 0; k < 4; ++k) reinterpret_cast<float4*>(s_U)[tid + k * 256] = u[k];
    }
    store_input();

    // 5x5: the 7th K step would carry ONE tap (row 4, column 4) in a 4-deep MFMA -- 32 pipe cycles for 64 useful FMAs per lane group.  That tap goes
    // to the VALU instead: every lane reads the input value under its own pixel and adds w[oc][24] * x to its four accumulators (4 FMAs, ~10 cycles)
    #ifdef SNNHIP_ESPCN_TAP25_MFMA // experiment builds (tools/exp_one.sh): the round-3 form, all 7 steps on the matrix pipe
    constexpr bool kValuTap = false;
#else
    constexpr bool kValuTap = K1 == 5;
#endif
    constexpr int KSM = kValuTap ? KS1 - 1 : KS1; // K steps on the matrix pipe
    float a1[KSM];
#pragma unroll
    for (int s = 0; s < KSM; ++s) a1[s] = wA1[s * 64 + lane];
    float sc1[4], sh1[4], sc2[4], sh2[4], w24[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sc1[r] = ep1[(4 * g + r) * 2];
        sh1[r] = ep1[(4 * g + r) * 2 + 1];
        sc2[r] = ep2[(4 * g + r) * 2];
        sh2[r] = ep2[(4 * g + r) * 2 + 1];
        w24[r] = kValuTap ? wA1[(KS1 - 1) * 64 + 4 * g + r] : 0.0f; // step 6 holds w[oc][24] at lane oc (its lane group 0)
    }
    const int rowTap = (g < K1 ? g : 0) * INP; // K-steps s < K1: tap row g (invalid g: zero weight, any initialised row)
    const int lastTap = 4 * INP + g;           // K-steps s >= K1 (K1 == 5): tap row 4, col g (+4)
    SNNHIP_STAMP(1);
    __syncthreads();
    SNNHIP_STAMP(2);

  for (;;) {
    int n, x0, y0;
    tile_origin(tile, n, x0, y0);
    const int next = tile + gridDim.x;
    const bool more = next < ntiles;
    // The two blocks of a CU (b and b + grid / 2: workgroups fill every CU's first slot before any second one) take turns at the higher wave priority,
    // tile by tile -- conv2d_widep_f16.hip's rule, measured here as well: kernel A 75.4 -> 73.5 us in six of six ABAB pairs on one box (round 5), the
    // headline 9.26 k -> 9.41 k images/s there.  Recorded as measured, not derived
#ifndef SNNHIP_ESPCN_NO_PRIO_ALT // (experiment builds switch it off)
    if (((tile / static_cast<int>(gridDim.x)) + (blockIdx.x >= (gridDim.x >> 1) ? 1 : 0)) & 1) __builtin_amdgcn_s_setprio(2);
    else __builtin_amdgcn_s_setprio(0);
#endif
    if (more) issue_loads(next);
    const bool border = x0 == 0 || y0 == 0 || x0 + TW >= p.W || y0 + TH >= p.H; // wave-uniform

    // ---- phase 1: conv1 over the C1H x C1W region, pixels flattened into 16-wide groups; wave wv owns groups
    // [wv*GPW, wv*GPW+GPW), two per iteration (two independent MFMA chains).  The LDS operands of iteration it+1 are
    // fetched before the MFMAs of iteration it (the loop is fully unrolled, so this is register renaming, not copies).
    {
        float bv[2][U][KS1]; // (5x5: slot KS1 - 1 holds the input value of the VALU tap)
        int rr[2][U], cc[2][U];
        bool valid[2][U];
        auto fetch = [&](int it, int buf) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int grp = wv * GPW + it * U + u;
                const int pi = grp * 16 + px;
                valid[buf][u] = (it * U + u < GPW) && pi < C1H * C1W;
                const int pc = valid[buf][u] ? pi : 0;
                rr[buf][u] = pc / C1W;
                cc[buf][u] = pc - rr[buf][u] * C1W;
                const float* src = s_in + rr[buf][u] * INP + cc[buf][u];
                const float* srcRow = src + rowTap;
#pragma unroll
                for (int s = 0; s < KSM; ++s) bv[buf][u][s] = s < K1 ? srcRow[s] : src[lastTap + 4 * (s - K1)];
                if (kValuTap) bv[buf][u][KS1 - 1] = src[4 * INP + 4]; // tap (4, 4) under this lane's pixel, whatever its lane group
            }
        };
        fetch(0, 0);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int cur = it & 1;
            if (it + 1 < NIT) fetch(it + 1, cur ^ 1);
            f32x4 acc[U];
#pragma unroll
            for (int u = 0; u < U; ++u) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[0], bv[cur][u][0], f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
#pragma unroll
            for (int s = 1; s < KSM; ++s)
#pragma unroll
                for (int u = 0; u < U; ++u) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[s], bv[cur][u][s], acc[u], 0, 0, 0);
            if (kValuTap) {
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[u][k] = fmaf(w24[k], bv[cur][u][KS1 - 1], acc[u][k]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float4 o;
                o.x = act_mode<AM>(p.act1, fmaf(acc[u][0], sc1[0], sh1[0]));
                o.y = act_mode<AM>(p.act1, fmaf(acc[u][1], sc1[1], sh1[1]));
                o.z = act_mode<AM>(p.act1, fmaf(acc[u][2], sc1[2], sh1[2]));
                o.w = act_mode<AM>(p.act1, fmaf(acc[u][3], sc1[3], sh1[3]));
                if (border) { // only tiles on the image border have conv1 pixels outside the image: they are conv2's zero padding
                    const int gy = y0 - 1 + rr[cur][u], gx = x0 - 1 + cc[cur][u];
                    if (!(gy >= 0 && gy < p.H && gx >= 0 && gx < p.W)) o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
                if (valid[cur][u]) {
                    const int c = cc[cur][u];
                    const int pl = rr[cur][u] * C1P + (c & 1) * HALFP + (c >> 1);
                    const int slot = g ^ (((pl >> 2) & 1) << 1);
                    *reinterpret_cast<float4*>(s_c1 + pl * 16 + slot * 4) = o;
                }
            }
        }
    }
    SNNHIP_STAMP(3);
    __syncthreads(); // c1 complete; every wave is done reading s_in
    if (more) store_input();
    SNNHIP_STAMP(4);

    // ---- phase 2: Winograd conv2.  Lane = (tile column t = px, channel quad g).
    // c1 pixel (r, c) lives at linear pixel pl = r*C1P + (c&1)*HALFP + (c>>1), 16-byte slot  q ^ 2*((pl>>2)&1).
    // Patch element (i, j) of tile (trow, t): pl = (2 trow + i)*C1P + (j&1)*HALFP + t + (j>>1).  C1P = 40 leaves bit 2 of
    // pl alone, HALFP = 20 flips it, so the swizzle term is one of two per-lane values and everything else is an
    // immediate offset: 4 address registers serve all 16 patch loads.
    const float* uBase = s_U + (px * 4 + (g ^ (((px >> 2) & 1) << 1))) * 4; // + pos*256: U[pos][oc = px][ic = 4g..4g+3]
    const float* dBase[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = px + (j >> 1);
        const int slot = g ^ ((((t >> 2) & 1) ^ (j & 1)) << 1);
        dBase[j] = s_c1 + (wv * (2 * GROUPS2) * C1P + (j & 1) * HALFP + t) * 16 + slot * 4;
    }
    float* yn = y + static_cast<size_t>(n) * p.H * p.W * 16;
#pragma unroll
    for (int gi = 0; gi < GROUPS2; ++gi) {
        const int trow = wv * GROUPS2 + gi; // tile row: output rows 2*trow, 2*trow+1; patch rows 2*trow .. 2*trow+3 of the c1 tile
        f32x4 d[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) d[i][j] = *reinterpret_cast<const f32x4*>(dBase[j] + (2 * gi + i) * C1P * 16);
        f32x4 Y[2][2];
#pragma unroll
        for (int nu = 0; nu < 4; ++nu) {
            // (d B)[:, nu], then V[xi] = (Bt (dB))[xi]
            f32x4 e[4], V[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                e[i] = nu == 0 ? d[i][0] - d[i][2] : nu == 1 ? d[i][1] + d[i][2] : nu == 2 ? d[i][2] - d[i][1] : d[i][1] - d[i][3];
            V[0] = e[0] - e[2];
            V[1] = e[1] + e[2];
            V[2] = e[2] - e[1];
            V[3] = e[1] - e[3];
            f32x4 u4[4], m[4];
#pragma unroll
            for (int xi = 0; xi < 4; ++xi) u4[xi] = *reinterpret_cast<const f32x4*>(uBase + (xi * 4 + nu) * 256);
#pragma unroll
            for (int xi = 0; xi < 4; ++xi) m[xi] = __builtin_amdgcn_mfma_f32_16x16x4f32(u4[xi][0], V[xi][0], f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
#pragma unroll
            for (int kk = 1; kk < 4; ++kk)
#pragma unroll
                for (int xi = 0; xi < 4; ++xi) m[xi] = __builtin_amdgcn_mfma_f32_16x16x4f32(u4[xi][kk], V[xi][kk], m[xi], 0, 0, 0);
            // output transform: T[a] = (At M)[a][nu];  Y[a][b] += T[a] * At[b][nu]
            const f32x4 T0 = m[0] + m[1] + m[2];
            const f32x4 T1 = m[1] - m[2] - m[3];
            if (nu == 0) {
                Y[0][0] = T0;
                Y[1][0] = T1;
            } else if (nu == 1) {
                Y[0][0] += T0;
                Y[1][0] += T1;
                Y[0][1] = T0;
                Y[1][1] = T1;
            } else if (nu == 2) {
                Y[0][0] += T0;
                Y[1][0] += T1;
                Y[0][1] -= T0;
                Y[1][1] -= T1;
            } else {
                Y[0][1] -= T0;
                Y[1][1] -= T1;
            }
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
                const int gy = y0 + 2 * trow + a, gx = x0 + 2 * px + bb;
                if (!border || (gy < p.H && gx < p.W)) {
                    float4 o;
                    o.x = act_mode<AM>(p.act2, fmaf(Y[a][bb][0], sc2[0], sh2[0]));
                    o.y = act_mode<AM>(p.act2, fmaf(Y[a][bb][1], sc2[1], sh2[1]));
                    o.z = act_mode<AM>(p.act2, fmaf(Y[a][bb][2], sc2[2], sh2[2]));
                    o.w = act_mode<AM>(p.act2, fmaf(Y[a][bb][3], sc2[3], sh2[3]));
                    *reinterpret_cast<float4*>(yn + (static_cast<size_t>(gy) * p.W + gx) * 16 + g * 4) = o;
                }
            }
    }
    SNNHIP_STAMP(5);
    if (!more) break;
    __syncthreads(); // c1 consumed, next input tile visible
    tile = next;
  }
    SNNHIP_STAMP(6);
