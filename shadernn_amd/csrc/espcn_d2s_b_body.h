// espcn_d2s_b_body.h -- the body of kernel B's direct form (espcn_fused.hip; the rules are chain_fuse.hip's), #included by its three kernels: rule B's (TOut = float), rule B8's
// (TOut = unsigned char: the epilogue quantises with quantize_u8(o, qout.scale, qout.offset), snnhip_u8_out_plan_create's map, and stores two
// 2-byte pairs instead of two float2) and the 16-bit form (TOut = unsigned short: quantize_u16(o, ...) << shift, snnhip_u16_out_plan_create's map,
// two 4-byte pairs; element 2gy*2W + 2gx is even, so both are aligned).  Textual inclusion for the reason espcn_wino_a_body.h gives.  In scope: TW,
// TH, SIMPLE, the type TOut, the kernel arguments p, qout, qout16 (each a constant dummy where the kernel has no such frame), x, w, ep, y.
    // LDS tile as four channel-quad PLANES, s_x[q][pixel] float4: a wave's 64 pixels (2 rows x 32) read 512 contiguous bytes per row from one
    // plane -- conflict-free without a swizzle -- and every operand address of the tap loop is ONE per-thread base + a wave-uniform tap offset + a
    // compile-time plane offset.  (The kernel is VALU-issue bound: rocprofv3 counted 708 VALU instructions per wave of which 288 are the
    // packed FMAs; the previous [pixel][quad ^ swizzle] layout spent 21 VALU instructions per tap on addresses, this one 2.)
    constexpr int TWH = TW + 2, THH = TH + 2, PLANE = THH * TWH * 4; // floats per plane
    static_assert(TW * TH == 256, "one thread per pixel");
    __shared__ __attribute__((aligned(16))) float s_x[4 * PLANE];

    const int tid = threadIdx.x;
    // tile decode on the scalar unit: the divisions by tilesX / tilesY are mul-hi by host-computed magic numbers (a run-time integer division of
    // a uniform value still compiles to ~20 VALU instructions of float reciprocal arithmetic, and this kernel is VALU-issue bound)
    const unsigned bid = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(xcd_tile_order(blockIdx.x, gridDim.x)));
    const unsigned bq = p.tilesX == 1 ? bid : __umulhi(bid, p.magicX);
    const int tx = static_cast<int>(bid - bq * p.tilesX);
    const unsigned n_u = p.tilesY == 1 ? bq : __umulhi(bq, p.magicY);
    const int ty = static_cast<int>(bq - n_u * p.tilesY), n = static_cast<int>(n_u);
    const int x0 = tx * TW, y0 = ty * TH;
    const float* xn = x + static_cast<size_t>(n) * p.H * p.W * 16;

    {
        const bool interior = x0 >= 1 && y0 >= 1 && x0 + TW + 1 <= p.W && y0 + TH + 1 <= p.H; // block-uniform: 95 % of the tiles at 1080p
        if (interior) {
            // no bounds tests, no zero fill, no index arithmetic: thread t < 4*TWH owns float4 t of EVERY halo row (a row of the tile is 4*TWH
            // contiguous float4 in memory), so its THH loads are one pointer walked by the image pitch and its THH LDS stores one offset walked by
            // the tile pitch.  The other threads (the fourth wave entirely) skip the staging: fewer instructions issued in total is what counts.
            if (tid < 4 * TWH) {
                const float* src = xn + (static_cast<size_t>(y0 - 1) * p.W + (x0 - 1)) * 16 + tid * 4;
                float4 rowv[THH];
#pragma unroll
                for (int rr = 0; rr < THH; ++rr) rowv[rr] = *reinterpret_cast<const float4*>(src + static_cast<size_t>(rr) * p.W * 16);
                float* dst = s_x + (tid & 3) * PLANE + (tid >> 2) * 4;
#pragma unroll
                for (int rr = 0; rr < THH; ++rr) *reinterpret_cast<float4*>(dst + rr * TWH * 4) = rowv[rr];
            }
        } else {
            constexpr int NLD = (THH * TWH * 4 + 255) / 256;
            float4 v[NLD];
#pragma unroll
            for (int k = 0; k < NLD; ++k) { // every load of the halo tile is in flight before the first LDS write
                const int idx = tid + k * 256;
                const int q = idx & 3, pix = idx >> 2;
                const int r = pix / TWH, c = pix - r * TWH;
                const int gy = y0 - 1 + r, gx = x0 - 1 + c;
                v[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (idx < THH * TWH * 4 && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W)
                    v[k] = *reinterpret_cast<const float4*>(xn + (static_cast<size_t>(gy) * p.W + gx) * 16 + q * 4);
            }
#pragma unroll
            for (int k = 0; k < NLD; ++k) {
                const int idx = tid + k * 256;
                if (idx < THH * TWH * 4) *reinterpret_cast<float4*>(s_x + (idx & 3) * PLANE + (idx >> 2) * 4) = v[k];
            }
        }
    }
    __syncthreads();

    const int c = tid % TW, r = tid / TW;
    // Packed fp32 FMAs: a wave64 v_fma_f32 occupies the VALU for 4 cycles on this kernel (measured: 20.3 M VALU instructions
    // = 20.6 M quad-cycles busy), v_pk_fma_f32 retires two FMAs per lane in the same slot.  The accumulators are kept as two
    // float2 so that every FMA is a v_pk_fma_f32 with the weight pair in an SGPR pair.
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    f32x2 acc01 = {0.0f, 0.0f}, acc23 = {0.0f, 0.0f};
    const float* base = s_x + (r * TWH + c) * 4;
    // one tap (64 uniform weights = 64 SGPRs) per iteration: unrolling further only spills SGPRs.  (Prefetching tap t+1's operand quads from
    // LDS does not pay: LDS and scalar loads share lgkmcnt, so the wait for the next weights also waits for the prefetch.)
#pragma unroll 1
    for (int fy = 0; fy < 3; ++fy) {
#pragma unroll 1
        for (int fx = 0; fx < 3; ++fx) {
            const int tap = fy * 3 + fx;
            const float* src = base + (fy * TWH + fx) * 4; // wave-uniform offset
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 xv = *reinterpret_cast<const float4*>(src + q * PLANE); // compile-time plane offset -> ds_read_b128 offset:
                const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float* wr = w + (tap * 16 + q * 4 + i) * 4; // uniform address -> s_load
                    const f32x2 xx = {xs[i], xs[i]};
                    const f32x2 w01 = {wr[0], wr[1]}, w23 = {wr[2], wr[3]};
                    acc01 = __builtin_elementwise_fma(xx, w01, acc01);
                    acc23 = __builtin_elementwise_fma(xx, w23, acc23);
                }
            }
        }
    }
    const float acc[4] = {acc01.x, acc01.y, acc23.x, acc23.y};
    const int gy = y0 + r, gx = x0 + c;
    if (gy < p.H && gx < p.W) {
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = fast_tanh(apply_act<SIMPLE>(p.act, fmaf(acc[k], ep[2 * k], ep[2 * k + 1]), 0.0f));
        TOut* yn = y + static_cast<size_t>(n) * (2 * p.H) * (2 * p.W);
        // channel 2*dy+dx -> output pixel (2y+dy, 2x+dx)  (depth_to_space, fs_subpixel.glsl:41-64)
        if constexpr (FrameBits<TOut>::value == 16) {
            unsigned q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = quantize_u16(o[k], qout16.scale, qout16.offset, qout16.maxval) << qout16.shift;
            *reinterpret_cast<unsigned*>(yn + static_cast<size_t>(2 * gy) * (2 * p.W) + 2 * gx) = q[0] | (q[1] << 16);
            *reinterpret_cast<unsigned*>(yn + static_cast<size_t>(2 * gy + 1) * (2 * p.W) + 2 * gx) = q[2] | (q[3] << 16);
        } else if constexpr (FrameBits<TOut>::value == 8) {
            const unsigned q[4] = {quantize_u8(o[0], qout.scale, qout.offset), quantize_u8(o[1], qout.scale, qout.offset),
                                   quantize_u8(o[2], qout.scale, qout.offset), quantize_u8(o[3], qout.scale, qout.offset)};
            *reinterpret_cast<unsigned short*>(yn + static_cast<size_t>(2 * gy) * (2 * p.W) + 2 * gx) = static_cast<unsigned short>(q[0] | (q[1] << 8));
            *reinterpret_cast<unsigned short*>(yn + static_cast<size_t>(2 * gy + 1) * (2 * p.W) + 2 * gx) = static_cast<unsigned short>(q[2] | (q[3] << 8));
        } else {
            *reinterpret_cast<float2*>(yn + static_cast<size_t>(2 * gy) * (2 * p.W) + 2 * gx) = make_float2(o[0], o[1]);
            *reinterpret_cast<float2*>(yn + static_cast<size_t>(2 * gy + 1) * (2 * p.W) + 2 * gx) = make_float2(o[2], o[3]);
        }
    }
