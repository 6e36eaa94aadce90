// conv2d_wide_body.h -- the body of conv2d_wide_kernel and conv2d_wide_cat_kernel (conv2d_wide_f16.hip), included INSIDE both __global__ definitions: as a shared
// __device__ function the single-source instances came out with another schedule.  In scope at the include: the template parameters WM, WN, NT, C8, R, SIMPLE,
// the constants RES, CAT and POOL, and p, cp, pq (WidePoolParams: chain rule L, conv2d_wide_pool_kernel), ac, x, wp, epi, y.
    static_assert(WM * WN == 4, "4 waves per block");
    static_assert(!(CAT && RES), "the two-source form has no residual input");
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    constexpr int MT = 4;
    constexpr int PIX = 32 * MT * WM;
    constexpr int BN = 32 * NT * WN;
    constexpr int Q = 2 * C8;  // 16-byte slots per staged pixel
    constexpr int S = 9 * C8;  // K steps (16 channels each) per chunk
    // weight ring depth in K steps (divides S).  One step is MT * NT MFMAs: 256 cycles with NT = 2 -- three steps of lead cover an L2 round trip --
    // but only 128 with NT = 1, where a whole chunk's 9 steps are kept in flight (64 -> 32 @816x1376 b16: 1500 -> 1277 us; no change for NT = 2)
    constexpr int D = NT == 1 ? 9 : 3;
    constexpr int kTileW = 34; // staged tile width: the 32-pixel tile row + the 3x3 halo
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const int l32 = lane & 31, h = lane >> 5;

    const int mt = blockIdx.x;
#ifdef SNNHIP_WIDE_TRACE
    const bool wtrace = (blockIdx.x == 777 || blockIdx.x == 5000) && blockIdx.y == 0 && (tid == 0 || tid == 192);
    unsigned long long wstamp[8] = {};
#endif
    WIDE_MARK(0);
    const int tx = mt % p.tilesX, ty = (mt / p.tilesX) % p.tilesY, n = mt / (p.tilesX * p.tilesY);
    const int ox0 = tx << 5, oy0 = ty << p.THs;
    const int ix0 = ox0 - p.padx, iy0 = oy0 - p.pady;

    // ---- staging.  LDS-DMA (lds_dma16): element e = tid + 256 r lands at 16-byte LDS slot e of the buffer (lane-contiguous, the only
    // placement the instruction offers).  A pixel owns Q + 1 slots: Q of data and one of padding, so that the 32 pixels of an operand row sit
    // (Q + 1) * 16 bytes apart -- an odd number of 16-byte bank slots, conflict-free for ds_read_b128 without an XOR swizzle, and every tap /
    // channel-slot displacement is an immediate offset of the ds_read (with the swizzle of lds_off the unrolled loop kept 72 precomputed
    // addresses in registers and spilled).  Pixels outside the image (zero padding), the padding slots and the slots past the tile read a
    // block of zeros behind the packed weights.  No staging registers, no ds_write; the copy for chunk c+1 is issued at the top of chunk c
    // and waited for with a COUNTED vmcnt before the closing barrier (the weight ring's youngest loads stay in flight).
    // The source pixel of a staged pixel is separable -- its row depends on the tile row only, its column on the tile column only -- so the padding
    // / fused Pad / fused UpSampling resolution runs ONCE per tile row and column (52 threads, one coordinate each) into two small LDS tables, and
    // a thread's R elements are two look-ups each (resolved per element it was ~110 VALU instructions x R: as long as a quarter of the wave's MFMAs)
    constexpr int QP = Q + 1;
    float* const epiTab = smem + p.epiOfs; // (behind the staging buffers AND the epilogue's output tile) this block's BN rows of the epilogue table {bias, bnScale, bnMean, bnBeta}
    float* const biasTab = epiTab + 4 * BN; // the biases alone, contiguous: the four of a lane's channel run are one ds_read_b128
    int* const syTab = reinterpret_cast<int*>(biasTab + BN); // [tileH <= 32] pixel index of the source row's first pixel, -1 = outside (zeros)
    int* const sxTab = syTab + 32;                          // [kTileW] source column, -1 = outside
    float* const normTab = reinterpret_cast<float*>(sxTab + 40); // [2][IC] graph rule I: shift, mul of this block's image
    if (p.normShift)
        for (int i = tid; i < p.IC; i += 256) {
            normTab[i] = p.normShift[n * p.IC + i];
            normTab[p.IC + i] = p.normMul[n * p.IC + i];
        }
    if (tid < BN) {
        const float4 e4 = epi[blockIdx.y * BN + tid];
        reinterpret_cast<float4*>(epiTab)[tid] = e4;
        biasTab[tid] = e4.x;
    }
    if (tid >= 192 && tid < 192 + kTileW) {
        const int c = tid - 192;
        int sx = resolve_nobranch(ix0 + c, p.W, p.padMode);
        if (p.preMode) { // a pixel of the (virtual) padded image -> the source pixel the Pad layer would have copied (-1 stays -1: size <= 2^30)
            const int px = resolve_nobranch(sx - p.preX, p.srcW << p.preShift, p.preMode);
            sx = sx < 0 ? -1 : (px < 0 ? -1 : px >> p.preShift);
        }
        sxTab[c] = sx;
    } else if (tid >= 128 && tid < 128 + p.tileH) {
        const int rr = tid - 128;
        int sy = resolve_nobranch(iy0 + rr, p.H, p.padMode);
        if (p.preMode) {
            const int py = resolve_nobranch(sy - p.preY, p.srcH << p.preShift, p.preMode);
            sy = sy < 0 ? -1 : (py < 0 ? -1 : py >> p.preShift);
        }
        syTab[rr] = sy < 0 ? -1 : (n * p.srcH + sy) * p.srcW;
    }
    __syncthreads();
    int gofs[R];
    unsigned qlPack = 0; // channel slot of element r in bits 4r .. 4r+2 (the norm fix-up below)
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = tid + 256 * r;
        gofs[r] = -1;
        if (e < p.total) {
            const int pix = e / QP;
            const int ql = e - pix * QP;
            qlPack |= static_cast<unsigned>(ql) << (4 * r);
            const int rr = static_cast<int>(__umulhi(static_cast<unsigned>(pix), p.magicW));
            const int c = pix - rr * p.tileW;
            const int rowPix = syTab[rr], sx = sxTab[c];
            if (rowPix >= 0 && sx >= 0 && ql < Q) gofs[r] = CAT ? rowPix + sx : (rowPix + sx) * p.IC + ql * 8; // (CAT: the pixel index, common to both sources)
        }
    }
    const _Float16* const zeros = reinterpret_cast<const _Float16*>(wp + p.zeroOfs);
    auto stage_dma = [&](float* buf, int ic0) {
        // CAT (uniform): the chunk's source, its pitch and the chunk's first channel in it
        const bool second = CAT && ic0 >= cp.C0;
        const _Float16* const xs = second ? cp.x1 : x;
        const int pitch = second ? p.IC - cp.C0 : cp.C0, rel = second ? ic0 - cp.C0 : ic0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const _Float16* src;
            if (CAT) src = gofs[r] >= 0 ? xs + (gofs[r] * pitch + 8 * static_cast<int>((qlPack >> (4 * r)) & 7u) + rel) : zeros; // one address, one load: never two
            else src = gofs[r] >= 0 ? x + gofs[r] + ic0 : zeros;
            lds_dma16(src, buf + (wave * 64 + 256 * r) * 4);
        }
    };

    // graph rule I: the DMA cannot touch the values it carries, so the InstanceNorm in front of this layer is applied to the chunk IN LDS: every
    // thread normalises exactly the 16-byte slots ITS lanes of the DMA wrote (no other thread has seen them: the pass sits between the DMA's
    // vmcnt wait and the barrier that publishes the chunk), x -> half(act(x * mul[c] + shift[c])) in fp32 -- the arithmetic and rounding point of
    // the norm's own normalise sweep, so the result is bit-identical to the separate launches.  Padding (zeros block) stays zero.  Costs ~180
    // instructions per thread and chunk next to the chunk's 144 MFMAs (+10 %); the normalise sweep it replaces is a read + write of the tensor.
    auto norm_fixup = [&](float* buf, int ic0) {
        typedef _Float16 h8v __attribute__((ext_vector_type(8)));
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (gofs[r] < 0) continue;
            float* slot = buf + (tid + 256 * r) * 4;
            const float* tb = normTab + ic0 + 8 * static_cast<int>((qlPack >> (4 * r)) & 7u);
            h8v hv = *reinterpret_cast<const h8v*>(slot);
#pragma unroll
            for (int q4 = 0; q4 < 2; ++q4) {
                const float4 sh = *reinterpret_cast<const float4*>(tb + 4 * q4), mu = *reinterpret_cast<const float4*>(tb + p.IC + 4 * q4);
                const float shv[4] = {sh.x, sh.y, sh.z, sh.w}, muv[4] = {mu.x, mu.y, mu.z, mu.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float f = fmaf(static_cast<float>(hv[4 * q4 + k]), muv[k], shv[k]);
                    // (one branch-free form for every simple activation -- ReLU is alpha 1, lo 0 --: a per-value select between this and fmaxf(f, 0) computed both)
                    hv[4 * q4 + k] = static_cast<_Float16>(__builtin_amdgcn_fmed3f(fmaxf(f, f * p.normAc.alpha), p.normAc.lo, p.normAc.hi));
                }
            }
            *reinterpret_cast<h8v*>(slot) = hv;
        }
    };

    // ---- MFMA operand addressing: lane (l32, h) reads pixel (row wm*MT + t of the tile, column l32), slot 2 c8 + h; aoff = float offset
    int aoff[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) aoff[t] = (((wm * MT + t) * p.tileW + l32) * QP + h) * 4;
    const int n0 = blockIdx.y * BN + wn * (NT * 32);
    const size_t bstep = static_cast<size_t>(2) * p.OCp; // float4 units per K step
    const float4* bptr = wp + (static_cast<size_t>(h) * p.OCp + n0 + l32);

    f32x16 acc[MT][NT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.0f;

    float4 bq[D][NT];
#pragma unroll
    for (int d = 0; d < D; ++d) {
#pragma unroll
        for (int u = 0; u < NT; ++u) bq[d][u] = bptr[u * 32];
        bptr += bstep;
    }

    WIDE_MARK(1);
    stage_dma(smem, 0);
    lds_dma_wait();
    if (p.normShift) norm_fixup(smem, 0);
    unsigned* const tok = p.kTok ? p.kTok + physical_cu_slot() : nullptr;
    if (tok && tid == 0) { // chunk 0 is in LDS: wait for the CU's other block to leave its K loop
        while (__hip_atomic_exchange(tok, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) __builtin_amdgcn_s_sleep(16);
    }
    __syncthreads();
    WIDE_MARK(2);

    float4 a[MT];
    for (int chunk = 0; chunk < p.nChunks; ++chunk) {
        const float* cur = smem + (chunk & 1) * p.bufFloats;
        const bool more = chunk + 1 < p.nChunks;
        if (more && !(SNNHIP_WIDE_ABL & 4)) stage_dma(smem + ((chunk + 1) & 1) * p.bufFloats, (chunk + 1) * 16 * C8);
#pragma unroll
        for (int t = 0; t < MT; ++t) a[t] = *reinterpret_cast<const float4*>(cur + aoff[t]);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            float4 b[NT];
#pragma unroll
            for (int u = 0; u < NT; ++u) b[u] = bq[s % D][u];
            if (!(SNNHIP_WIDE_ABL & 1)) {
#pragma unroll
                for (int u = 0; u < NT; ++u) bq[s % D][u] = bptr[u * 32];
                bptr += bstep;
            }
            __builtin_amdgcn_sched_barrier(0); // the refill stays D steps ahead of its use
            const int tap = (s + 1) / C8;
            const int dl = (((tap / 3) * kTileW + (tap % 3)) * QP + ((s + 1) % C8) * 2) * 4; // compile-time: an immediate offset of the ds_read
            // pixel-tile major: a[t] is dead after its NT MFMAs and is refilled for the next step at once -- no second operand set in registers
#pragma unroll
            for (int t = 0; t < MT; ++t) {
#pragma unroll
                for (int u = 0; u < NT; ++u)
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const h8*>(&b[u]), *reinterpret_cast<const h8*>(&a[t]), acc[t][u], 0, 0, 0);
                if (s + 1 < S && !(SNNHIP_WIDE_ABL & 2)) a[t] = *reinterpret_cast<const float4*>(cur + aoff[t] + dl);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // the DMA of this chunk is older than every weight refill of the chunk; the ring keeps D * NT loads in flight
        if (D * NT == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else if (D * NT == 9) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        if (p.normShift && more) norm_fixup(smem + ((chunk + 1) & 1) * p.bufFloats, (chunk + 1) * 16 * C8);
        __syncthreads();
    }

    if (tok && tid == 0) __hip_atomic_store(tok, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    WIDE_MARK(3);
    // ---- epilogue.  The MFMAs ran with the WEIGHTS as the A operand (M = output channels) and the pixels as B (N = 32 pixels of a tile row), so
    // a lane holds, for ITS pixel, runs of four consecutive output channels: acc[t][u][4g + k] = channel n0 + 32u + 8g + 4h + k of pixel
    // (row wm*MT + t, column l32).  bias -> BN -> activation, each run goes to the LDS tile [pixel][BN halfs] as ONE ds_write_b64 (with the
    // pixels in the accumulator rows it took 128 ds_write_b16 per wave and the epilogue ran as long as the block's MFMAs); the tile then leaves
    // as 16-byte vectors, a pixel's BN channels contiguous (whole 128-byte lines -- storing the 8-byte runs directly was measured 10 % slower
    // than this round trip: 32 partial lines per store instruction).  The fused residual Add (RES) is added to the fp32 values, in front of
    // the one rounding; its loads are all issued before the first store (gfx9 counts loads and stores in one vmcnt and retires them out of order
    // with respect to each other: a load behind a store can only be waited for with vmcnt(0), the full write round trip).
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    constexpr int EPITCH = BN + 8; // halfs per pixel row of the LDS tile: 8-byte runs of 16 consecutive pixels land in distinct banks
    _Float16* const otile = reinterpret_cast<_Float16*>(smem);
    const float4* const etab = reinterpret_cast<const float4*>(epiTab) + wn * (NT * 32) + 4 * h;
    // layers without batch norm (all of the style graphs): the lane's 8 NT biases are read BEFORE the first write of the output tile -- the
    // compiler cannot tell the table from the tile (one LDS array) and serialises a read - wait - write round trip per channel run otherwise
    float4 bias4[NT][4];
    if (!p.useBN) {
        const float4* const btab = reinterpret_cast<const float4*>(biasTab + wn * (NT * 32) + 4 * h);
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
            for (int g = 0; g < 4; ++g) bias4[u][g] = btab[u * 8 + 2 * g];
    }
    // layers without batch norm whose activation is none or relu (every 3x3 layer of the style graphs): bias and clamp, two instructions per value --
    // the general form below (run-time batch-norm select, mul / max / med3 activation) is seven, and with 128 values per lane the epilogue's
    // VALU work was a third of the wave's MFMA time
    const bool fastEpi = SIMPLE && !p.useBN && ac.alpha == 1.0f && ac.hi == __builtin_huge_valf();
    if (POOL) {
        // ---- chain rule L: MaxPooling2D 2x2 stride 2 behind the epilogue, a two-stage maximum.  The tile's rows start even (oy0 = ty << THs) and MT = 4 is
        // even, so a window's two ROWS are the lane's accumulators t = 2 tp, 2 tp + 1; its two COLUMNS are in neighbouring lanes.
        // Stage 1, registers: bias -> BN -> activation in fp32 on both rows (BN's scale may be negative: the maximum stays behind it), the pooling plan's own
        // rule m = -100000, m = max(m, v) over the rows inside OH, ONE rounding to half, one ds_write_b64 per channel run and row PAIR into the pooled-row tile
        // [PIX / 64 rows][32 columns][BN halfs]: half the plain epilogue's LDS writes.  Stage 2, read-out: the tile leaves as 16-byte vectors, each the packed
        // half maximum (v_pk_max_f16) of two adjacent pixels' vectors, the odd column only where it is inside OW.  Rounding to half is monotone, so
        // max(half(a), half(b)) = half(max(a, b)): the result is the separate launches', bit for bit.
        static_assert(!POOL || (MT % 2 == 0 && !RES && !CAT), "the pooling epilogue: whole row pairs per lane, one source, no residual");
        _Float16* const ptile = otile;
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float4 e[4];
                if (p.useBN) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) e[k] = etab[u * 32 + 8 * g + k];
                } else {
                    e[0].x = bias4[u][g].x; e[1].x = bias4[u][g].y; e[2].x = bias4[u][g].z; e[3].x = bias4[u][g].w;
                }
#pragma unroll
                for (int tp = 0; tp < MT / 2; ++tp) {
                    const bool in2 = oy0 + wm * MT + 2 * tp + 1 < p.OH; // (the first row is inside wherever the window is stored)
                    h4 o;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float m = -100000.0f;
#pragma unroll
                        for (int r = 0; r < 2; ++r) {
                            const float a = acc[2 * tp + r][u][4 * g + k];
                            const float v = fastEpi ? fmaxf(a + e[k].x, ac.lo) : apply_act<true>(ac, epi_affine(a, e[k], p.useBN), 0.0f); // (the plain epilogue's two forms)
                            if (r == 0 || in2) m = fmaxf(m, v);
                        }
                        o[k] = static_cast<_Float16>(m);
                    }
                    *reinterpret_cast<h4*>(ptile + ((wm * (MT / 2) + tp) * 32 + l32) * EPITCH + wn * (NT * 32) + u * 32 + 8 * g + 4 * h) = o;
                }
            }
        __syncthreads();
        constexpr int PVPR = BN / 8;                    // 16-byte vectors per pooled pixel
        constexpr int PNV = (PIX / 4) * PVPR / 256;     // ... per thread: PIX / 4 windows per tile
#pragma unroll
        for (int j = 0; j < PNV; ++j) {
            const int v = tid + 256 * j;
            const int i = v / PVPR, c8 = v - i * PVPR; // window i = (pooled row i >> 4, pooled column i & 15) of the tile
            const int pr = i >> 4, pc = i & 15;
            const int oy = oy0 + 2 * pr, ox = ox0 + 2 * pc, qy = oy >> 1, qx = ox >> 1;
            const h8 a = *reinterpret_cast<const h8*>(ptile + (pr * 32 + 2 * pc) * EPITCH + c8 * 8);
            const h8 b = *reinterpret_cast<const h8*>(ptile + (pr * 32 + 2 * pc + 1) * EPITCH + c8 * 8);
            const h8 m = ox + 1 < p.OW ? __builtin_elementwise_max(a, b) : a;
            if (oy < p.OH && ox < p.OW && qy < pq.poolOH && qx < pq.poolOW)
                *reinterpret_cast<h8*>(y + static_cast<size_t>((n * pq.poolOH + qy) * pq.poolOW + qx) * p.OC + blockIdx.y * BN + c8 * 8) = m;
        }
        return;
    }
    constexpr int VPR = BN / 8;             // 16-byte vectors per pixel of the tile
    constexpr int NV = PIX * VPR / 256;     // ... per thread
    int oofs[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int v = tid + 256 * j;
        const int i = v / VPR, c8 = v - i * VPR;
        const int oy = oy0 + (i >> 5), ox = ox0 + (i & 31);
        oofs[j] = (oy < p.OH && ox < p.OW) ? ((n * p.OH + oy) * p.OW + ox) * p.OC + blockIdx.y * BN + c8 * 8 : -1;
    }
    if (RES) { // the residual comes in through the tile, transposed the other way: its 16-byte vectors land where the result will stand (the K loop ended
               // on a barrier: the staging buffers under the tile are dead), and every lane below adds the run it is about to overwrite to its fp32 values
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int v = tid + 256 * j;
            const int i = v / VPR, c8 = v - i * VPR;
            *reinterpret_cast<float4*>(otile + i * EPITCH + c8 * 8) =
                oofs[j] >= 0 ? *reinterpret_cast<const float4*>(static_cast<const _Float16*>(p.res) + oofs[j]) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
    }
    if (fastEpi) {
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float bk[4] = {bias4[u][g].x, bias4[u][g].y, bias4[u][g].z, bias4[u][g].w};
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    h4* const slot = reinterpret_cast<h4*>(otile + ((wm * MT + t) * 32 + l32) * EPITCH + wn * (NT * 32) + u * 32 + 8 * g + 4 * h);
                    h4 o, r;
                    if (RES) r = *slot;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float v = fmaxf(acc[t][u][4 * g + k] + bk[k], ac.lo);
                        if (RES) v = add_act(p.ac2, true, v + static_cast<float>(r[k]));
                        o[k] = static_cast<_Float16>(v);
                    }
                    *slot = o;
                }
            }
    } else
#pragma unroll
    for (int u = 0; u < NT; ++u)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float4 e[4];
            if (p.useBN) {
#pragma unroll
                for (int k = 0; k < 4; ++k) e[k] = etab[u * 32 + 8 * g + k];
            } else {
                e[0].x = bias4[u][g].x; e[1].x = bias4[u][g].y; e[2].x = bias4[u][g].z; e[3].x = bias4[u][g].w;
            }
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                h4* const slot = reinterpret_cast<h4*>(otile + ((wm * MT + t) * 32 + l32) * EPITCH + wn * (NT * 32) + u * 32 + 8 * g + 4 * h);
                h4 o, r;
                if (RES) r = *slot;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float v = epi_affine(acc[t][u][4 * g + k], e[k], p.useBN);
                    v = SIMPLE ? apply_act<true>(ac, v, 0.0f) : epi_act(ac.act, ac.leaky, v, 0.0f);
                    if (RES) v = add_act(p.ac2, true, v + static_cast<float>(r[k])); // on the fp32 value: the store is the one rounding
                    o[k] = static_cast<_Float16>(v);
                }
                *slot = o;
            }
        }
    WIDE_MARK(4);
    __syncthreads();
    // chain rule F (p.statPart, uniform): the InstanceNorm behind this layer needs mean and variance per (image, channel).  A thread's NV vectors are
    // NV pixels of ONE 8-channel column (256 % VPR == 0): sums of (v - pivot) and (v - pivot)^2 of the stored (rounded) values accumulate in
    // registers while the vectors pass through, pivot = the thread's first pixel (the differences stay small: no cancellation in S2 - S1^2 / n)
    WIDE_MARK(5);
    float sPiv[8], sA[8], sB[8];
    int sCnt = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) sPiv[e] = sA[e] = sB[e] = 0.0f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int v = tid + 256 * j;
        const int i = v / VPR, c8 = v - i * VPR;
        float4 pack = *reinterpret_cast<const float4*>(otile + i * EPITCH + c8 * 8);
        if (!RES && p.statPart && oofs[j] >= 0) {
            const _Float16* ch = reinterpret_cast<const _Float16*>(&pack);
            if (sCnt == 0) {
#pragma unroll
                for (int e = 0; e < 8; ++e) sPiv[e] = static_cast<float>(ch[e]);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float f = static_cast<float>(ch[e]) - sPiv[e];
                sA[e] += f;
                sB[e] = fmaf(f, f, sB[e]);
            }
            ++sCnt;
        }
        if (oofs[j] >= 0 && !((SNNHIP_WIDE_ABL & 8) && p.OC != 12345)) *reinterpret_cast<float4*>(y + oofs[j]) = pack;
    }
    WIDE_MARK(6);
#ifdef SNNHIP_WIDE_TRACE
    if (wtrace && !(!RES && p.statPart))
        printf("widetrace blk %d tid %d: prologue %llu stage0 %llu kloop %llu epi %llu bar %llu stores %llu total %llu\n", blockIdx.x, tid, wstamp[1] - wstamp[0], wstamp[2] - wstamp[1],
               wstamp[3] - wstamp[2], wstamp[4] - wstamp[3], wstamp[5] - wstamp[4], wstamp[6] - wstamp[5], wstamp[6] - wstamp[0]);
#endif
    if (!RES && p.statPart) {
        // thread record (count, mean, M2) per channel -> LDS (the output tile is dead); thread c < BN then merges the PG pixel groups of its channel in a
        // fixed order with the parallel-variance update (n = na + nb, d = mb - ma, m = ma + d nb / n, M2 = M2a + M2b + d^2 na nb / n): deterministic,
        // and as accurate as the two-pass form whatever the mean / deviation ratio of the layer
        constexpr int PG = 256 / VPR;
        float* const sred = smem; // [3][PG][BN]
        __syncthreads();
        {
            const int c8 = tid % VPR, pg = tid / VPR;
            const float cn = static_cast<float>(sCnt), inv = sCnt > 0 ? 1.0f / cn : 0.0f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float m1 = sA[e] * inv;
                sred[pg * BN + c8 * 8 + e] = sPiv[e] + m1;
                sred[(PG + pg) * BN + c8 * 8 + e] = fmaxf(sB[e] - sA[e] * m1, 0.0f);
            }
            if (c8 == 0) sred[2 * PG * BN + pg] = cn;
        }
        __syncthreads();
        // two levels, all loads ahead of the dependent arithmetic: thread (channel c, part q) merges 8 pixel groups, thread c < BN the 256 / BN parts
        // (one thread per channel walking all PG = 16..64 groups was a 64-step chain of LDS round trips and divisions: +60 % on the 32-channel blocks)
        constexpr int PARTS = 256 / BN, GP = PG / PARTS;
        float* const sred2 = sred + 2 * PG * BN + PG; // [3][PARTS][BN]
        {
            const int c = tid % BN, q = tid / BN;
            float nb[GP], mb[GP], qb[GP];
#pragma unroll
            for (int j = 0; j < GP; ++j) {
                nb[j] = sred[2 * PG * BN + q * GP + j];
                mb[j] = sred[(q * GP + j) * BN + c];
                qb[j] = sred[(PG + q * GP + j) * BN + c];
            }
            float na = 0.0f, ma = 0.0f, M2 = 0.0f;
#pragma unroll
            for (int j = 0; j < GP; ++j) {
                const float n2 = na + nb[j], d = mb[j] - ma, r = nb[j] * __builtin_amdgcn_rcpf(fmaxf(n2, 1.0f)); // nb = 0 (a group outside the image): no change
                ma = fmaf(d, r, ma);
                M2 += qb[j] + d * d * na * r;
                na = n2;
            }
            sred2[q * BN + c] = na;
            sred2[(PARTS + q) * BN + c] = ma;
            sred2[(2 * PARTS + q) * BN + c] = M2;
        }
        __syncthreads();
        if (tid < BN) {
            float nb[PARTS], mb[PARTS], qb[PARTS];
#pragma unroll
            for (int j = 0; j < PARTS; ++j) {
                nb[j] = sred2[j * BN + tid];
                mb[j] = sred2[(PARTS + j) * BN + tid];
                qb[j] = sred2[(2 * PARTS + j) * BN + tid];
            }
            float na = 0.0f, ma = 0.0f, M2 = 0.0f;
#pragma unroll
            for (int j = 0; j < PARTS; ++j) {
                const float n2 = na + nb[j], d = mb[j] - ma, r = nb[j] * __builtin_amdgcn_rcpf(fmaxf(n2, 1.0f));
                ma = fmaf(d, r, ma);
                M2 += qb[j] + d * d * na * r;
                na = n2;
            }
            float* po = p.statPart + (static_cast<size_t>(n * p.tilesY + ty) * p.tilesX + tx) * 2 * p.OC + blockIdx.y * BN;
            st_agent(po + tid, ma); // (read by another block of this launch when the kernel folds: norm_fold.h)
            st_agent(po + p.OC + tid, M2);
        }
        WIDE_MARK(7);
#ifdef SNNHIP_WIDE_TRACE
        if (wtrace)
            printf("widetrace blk %d tid %d: prologue %llu stage0 %llu kloop %llu epi %llu bar %llu stores %llu stats %llu total %llu\n", blockIdx.x, tid, wstamp[1] - wstamp[0],
                   wstamp[2] - wstamp[1], wstamp[3] - wstamp[2], wstamp[4] - wstamp[3], wstamp[5] - wstamp[4], wstamp[6] - wstamp[5], wstamp[7] - wstamp[6], wstamp[7] - wstamp[0]);
#endif
        if (p.fold.counter) tile_stats_finish<BN>(p.fold, p.statPart, sred2 + 3 * 256, n, p.tilesX, p.tilesY, 1 << p.THs, 32, p.OH, p.OW, p.OC, blockIdx.y * BN);
    }
