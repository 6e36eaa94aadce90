// espcn_d2s_mfma_body.h -- the body of chain rule B for upscale factors R = 3 and 4 (espcn_d2s_mfma.hip), #included by its three kernels: the fp32 one
// (TOut = float), rule B8's (TOut = unsigned char: the epilogue quantises with quantize_u8(o, qout.scale, qout.offset),
// snnhip_u8_out_plan_create's map) and the 16-bit form (TOut = unsigned short: quantize_u16(o, ...) << shift, snnhip_u16_out_plan_create's map).
// Textual inclusion for the reason espcn_wino_a_body.h gives.  In scope: R, SIMPLE, the type TOut, the kernel arguments p, qout, qout16 (each a
// constant dummy where the kernel has no such frame), x, w, ep, y.
//
// conv 3x3 (16 -> R*R, zero padding 1) + act, then depth-to-space(R) + tanh, as a GEMM on v_mfma_f32_16x16x4_f32 (true fp32 products):
//   D[row][pixel] += Wt[row][ic] * X[ic][pixel],  9 taps x 4 K-steps per group of 16 pixels, A operand = the weights (36 VGPRs, loaded once),
//   B operand = one ds_read_b128 (4 input channels of one pixel) -- rule A's conv2 loop (conv_kxk_c1o16_conv3x3_c16o16_kernel, phase 2).
// The 16 MFMA rows are NOT the channels in order: row 4*dy + dx holds channel R*dy + dx (the host packs w and ep that way; for R = 3 rows 3, 7,
// 11 and 12..15 are zero).  A lane's four accumulator registers are rows 4g .. 4g+3 of pixel px, so lane (px, g) ends up with the R consecutive
// pixels of output row R*y + g that its low-resolution pixel owns, and the 16 lanes of one g hold 16*R CONSECUTIVE pixels of that row: every
// store instruction of the epilogue writes R rows x 16*R contiguous elements, with no transposition through LDS.
//   R = 4: one 16-byte store per lane (256 B runs); bytes: one 4-byte store (64 B runs)
//   R = 3: one 12-byte store per lane (192 B runs); bytes: the four lanes of a pixel quad hold 12 bytes = 3 dwords, lane j < 3 of the quad
//          builds dword j from its own 3 bytes and its right neighbour's (one lane shift) -- 4-byte stores, 48 B runs.  That needs the row
//          pitch 3*W to be a multiple of 4 (every video width is); other widths store the three bytes one by one.
//   16-bit frames: R = 4: one 8-byte store per lane (element 4*(...) : always aligned).  R = 3: six bytes at a 2-byte-aligned address, element
//          9nHW + (3gy + g)*3W + 3gx: even -> a 4-byte store of pixels 0, 1 and a 2-byte store of pixel 2, odd -> 2 bytes, then 4 (the half epilogue of
//          espcn_f16.hip splits the same layout the same way).
// Tile = 32 x 8 low-resolution pixels, 256 threads = 4 waves, a wave owns 2 rows = 4 groups (accumulators); LDS = the 34 x 10 halo tile,
// [row][col][16 ch] with rule A's 16-byte-slot swizzle, 21.8 KB.
    constexpr int TW = kD2sMfmaTW, TH = kD2sMfmaTH, TWH = TW + 2, THH = TH + 2;
    constexpr int NF4 = THH * TWH * 4, NLD = (NF4 + 255) / 256; // float4 of the halo tile; per thread
    constexpr int G = 4;                                       // 16-pixel groups per wave: rows 2wv, 2wv+1 x column halves
    static_assert(TW == 32 && TH == 8, "a wave owns 2 rows of 32 pixels = four 16-pixel groups");
    static_assert(R == 3 || R == 4, "rows 4*dy + dx: R <= 4; R = 2 has its own kernel");
    __shared__ __attribute__((aligned(16))) float s_x[THH * TWH * 16];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int px = lane & 15, g = lane >> 4;
    // tile decode on the scalar unit (as espcn_d2s_b_body.h)
    const unsigned bid = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(xcd_tile_order(blockIdx.x, gridDim.x)));
    const unsigned bq = p.tilesX == 1 ? bid : __umulhi(bid, p.magicX);
    const int tx = static_cast<int>(bid - bq * p.tilesX);
    const unsigned n_u = p.tilesY == 1 ? bq : __umulhi(bq, p.magicY);
    const int ty = static_cast<int>(bq - n_u * p.tilesY), n = static_cast<int>(n_u);
    const int x0 = tx * TW, y0 = ty * TH;
    const float* xn = x + static_cast<size_t>(n) * p.H * p.W * 16;

    // ---- halo tile (origin y0-1, x0-1) -> LDS, zero outside the image (the convolution's padding)
    {
        float4 v[NLD];
#pragma unroll
        for (int k = 0; k < NLD; ++k) { // every load is in flight before the first LDS write
            const int idx = tid + k * 256;
            const int q = idx & 3, pix = idx >> 2;
            const int r = pix / TWH, c = pix - r * TWH;
            const int gy = y0 - 1 + r, gx = x0 - 1 + c;
            v[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (idx < NF4 && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W)
                v[k] = *reinterpret_cast<const float4*>(xn + (static_cast<size_t>(gy) * p.W + gx) * 16 + q * 4);
        }
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int idx = tid + k * 256;
            const int q = idx & 3, pix = idx >> 2;
            const int c = pix % TWH;
            const int slot = q ^ (((c >> 2) & 1) << 1);
            if (idx < NF4) *reinterpret_cast<float4*>(s_x + pix * 16 + slot * 4) = v[k];
        }
    }
    // ---- weights -> registers (the host packed them in lane order), epilogue (scale, shift) of this lane's four rows
    float a[36];
#pragma unroll
    for (int t = 0; t < 36; ++t) a[t] = w[t * 64 + lane];
    float sc[4], sh[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sc[r] = ep[(4 * g + r) * 2];
        sh[r] = ep[(4 * g + r) * 2 + 1];
    }
    __syncthreads();

    f32x4 acc[G];
#pragma unroll
    for (int gi = 0; gi < G; ++gi) acc[gi] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int fy = tap / 3, fx = tap % 3;
        float4 bv[G];
#pragma unroll
        for (int gi = 0; gi < G; ++gi) {
            const int row = wv * 2 + (gi >> 1), cc = (gi & 1) * 16 + px + fx;
            const int slot = g ^ (((cc >> 2) & 1) << 1);
            bv[gi] = *reinterpret_cast<const float4*>(s_x + ((row + fy) * TWH + cc) * 16 + slot * 4);
        }
        // four independent accumulation chains between two uses of the same accumulator
#pragma unroll
        for (int gi = 0; gi < G; ++gi) acc[gi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tap * 4 + 0], bv[gi].x, acc[gi], 0, 0, 0);
#pragma unroll
        for (int gi = 0; gi < G; ++gi) acc[gi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tap * 4 + 1], bv[gi].y, acc[gi], 0, 0, 0);
#pragma unroll
        for (int gi = 0; gi < G; ++gi) acc[gi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tap * 4 + 2], bv[gi].z, acc[gi], 0, 0, 0);
#pragma unroll
        for (int gi = 0; gi < G; ++gi) acc[gi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tap * 4 + 3], bv[gi].w, acc[gi], 0, 0, 0);
    }

    // ---- epilogue: bias/BN/act, tanh; lane (px, g < R) holds output row R*gy + g, columns R*gx .. R*gx + R-1
    TOut* yn = y + static_cast<size_t>(n) * (R * p.H) * (R * p.W);
    [[maybe_unused]] const bool dwordRows = (p.W & 3) == 0; // R = 3, bytes: every pixel quad starts on a 4-byte boundary
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
        const int gy = y0 + wv * 2 + (gi >> 1), gx = x0 + (gi & 1) * 16 + px;
        const bool ok = g < R && gy < p.H && gx < p.W;
        float o[R];
#pragma unroll
        for (int r = 0; r < R; ++r) o[r] = fast_tanh(apply_act<SIMPLE>(p.act, fmaf(acc[gi][r], sc[r], sh[r]), 0.0f));
        TOut* dst = yn + static_cast<size_t>(R * gy + g) * (R * p.W) + R * gx;
        if constexpr (FrameBits<TOut>::value == 16) {
            unsigned q[R];
#pragma unroll
            for (int r = 0; r < R; ++r) q[r] = quantize_u16(o[r], qout16.scale, qout16.offset, qout16.maxval) << qout16.shift;
            if constexpr (R == 4) {
                if (ok) *reinterpret_cast<uint2*>(dst) = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
            } else if (ok) {
                if ((reinterpret_cast<uintptr_t>(dst) & 2) == 0) {
                    *reinterpret_cast<unsigned*>(dst) = q[0] | (q[1] << 16);
                    dst[2] = static_cast<TOut>(q[2]);
                } else {
                    dst[0] = static_cast<TOut>(q[0]);
                    *reinterpret_cast<unsigned*>(dst + 1) = q[1] | (q[2] << 16);
                }
            }
        } else if constexpr (FrameBits<TOut>::value == 8) {
            unsigned v = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) v |= quantize_u8(o[r], qout.scale, qout.offset) << (8 * r);
            if constexpr (R == 4) {
                if (ok) *reinterpret_cast<unsigned*>(dst) = v;
            } else {
                const unsigned nb = __shfl_down(v, 1); // the right neighbour's three bytes (every lane takes part)
                const int j = px & 3;
                if (dwordRows) { // W % 4 == 0: a quad is inside the image or outside it as a whole
                    if (ok && j < 3) *reinterpret_cast<unsigned*>(dst + j) = (v >> (8 * j)) | (nb << (24 - 8 * j));
                } else if (ok) {
                    dst[0] = static_cast<unsigned char>(v);
                    dst[1] = static_cast<unsigned char>(v >> 8);
                    dst[2] = static_cast<unsigned char>(v >> 16);
                }
            }
        } else {
            if constexpr (R == 4) {
                if (ok) *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
                struct alignas(4) F3 {
                    float a, b, c;
                };
                if (ok) *reinterpret_cast<F3*>(dst) = F3{o[0], o[1], o[2]};
            }
        }
    }
