// conv2d_wino_body.h -- the body of conv2d_wino_kernel / conv2d_wino_cat_kernel / conv2d_wino_pool_kernel (conv2d_wino.hip), included INSIDE each of the three
// kernel definitions.  The includer provides: the template parameters SIMPLE, OPB, KS; constexpr bool CAT, POOL; the kernel arguments p, ac, x, ug, epi, y, ws; cp
// (WinoCatParams: the kernel argument of the CAT form, an empty block nobody reads otherwise) and pq (WinoPoolParams, likewise for POOL).  Text, not a function: the single-source kernels keep the
// instruction streams they had before the two-source form existed (an inlined __device__ body changed their schedule).
    static_assert(KS == 1 || (KS == 2 && OPB == 1), "in-block K split: two groups of four waves");
    constexpr int NT = 256 * OPB;            // threads of a group
    constexpr int kUFloats = 4096 * OPB;     // U slab of one chunk: 16 positions x OPB pairs x 64 lanes x float4 (16 / 32 KB)
    constexpr int UQ = 1024 * OPB;           // ... in float4
    constexpr int R = 4 / OPB;               // staged activation quads per thread (halo tile of up to 1024 quads)
    extern __shared__ __attribute__((aligned(16))) float smemAll[];
    const int lane = threadIdx.x & 63;
    const int ks = KS > 1 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 8) : 0; // K group of this wave
    const int tid = KS > 1 ? (threadIdx.x & 255) : threadIdx.x, wave = tid >> 6;     // thread / wave within the group
    float* const smem = smemAll + ks * 2 * p.bufFloats;                              // the group's two buffers
    const int tg = wave & 3, op = wave >> 2;
    const int n16 = lane & 15, k = lane >> 4;

    const int mt = blockIdx.x;
    const int tx = mt % p.tilesX, ty = (mt / p.tilesX) % p.tilesY, tb = mt / (p.tilesX * p.tilesY);
    const int TTW = 1 << p.TTWs, TTH = 1 << p.TTHs;
    const int ox0 = tx * 2 * TTW, oy0 = ty * 2 * TTH, b0 = tb << p.TBs;
    const int ix0 = ox0 - p.padx, iy0 = oy0 - p.pady;

    // ---- staging descriptors: element e = tid + NT r -> (pixel of the halo tile, channel quad q = e & 1)
    const int q = tid & 1;
    int gofs[4], lofs[4];
    // (CAT: pitch_ / srcH_ / srcW_ / sh_ describe the source the offsets are for; the bounds test is the convolution's own H x W for both)
#define WINO_DESCRIPTORS(pitch_, srcH_, srcW_, sh_)                                                                                            \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                                            \
        gofs[r] = lofs[r] = -1;                                                                                                                \
        if (r >= R) continue;                                                                                                                  \
        const int e = tid + NT * r;                                                                                                            \
        gofs[r] = -1;                                                                                                                          \
        lofs[r] = -1;                                                                                                                          \
        if (e < p.total) {                                                                                                                     \
            const int pix = e >> 1;                                                                                                            \
            const int c = pix % p.inW, t2 = pix / p.inW;                                                                                       \
            const int rr = t2 % p.inH, b = t2 / p.inH;                                                                                         \
            const int sy = iy0 + rr, sx = ix0 + c, n = b0 + b;                                                                                 \
            lofs[r] = kUFloats + 2 * q * p.planeStride + ((b * p.inH + rr) * p.rowPitch + c) * 2;                                              \
            if (sy >= 0 && sy < p.H && sx >= 0 && sx < p.W && n < p.N)                                                                         \
                gofs[r] = CAT ? ((n * (srcH_) + (sy >> (sh_))) * (srcW_) + (sx >> (sh_))) * (pitch_) + q * 4 : ((n * p.H + sy) * p.W + sx) * p.IC + q * 4; \
        }                                                                                                                                      \
    }
    if (!CAT) { WINO_DESCRIPTORS(p.IC, p.H, p.W, 0) }
    int chunk0 = blockIdx.z * p.chunksPerSplit, chunk1 = min(p.nChunks, chunk0 + p.chunksPerSplit);
    if (KS > 1) { // (the planner only splits even chunk counts: both groups run the same number of iterations, their barriers pair up)
        const int half = (chunk1 - chunk0) >> 1;
        chunk0 += ks * half;
        chunk1 = chunk0 + half;
    }
    // U slab of (oc block, chunk): UQ float4, thread t copies float4 t + NT j, j < 4
    const float4* uptr = ug + (static_cast<size_t>(blockIdx.y) * p.nChunks + chunk0) * UQ + tid;
    // CAT: the source of the range's first chunk (a blockIdx.z slice or the second K group may begin inside input 1)
    const float* xs = x;
    int chunkOrg = 0;
#define WINO_SET_SOURCE(one_)                                                  \
    do {                                                                       \
        if (one_) {                                                            \
            xs = cp.x1;                                                        \
            chunkOrg = cp.c0Chunks;                                            \
            WINO_DESCRIPTORS(cp.pitch1, p.H, p.W, 0)                           \
        } else {                                                               \
            WINO_DESCRIPTORS(cp.pitch0, cp.srcH, cp.srcW, cp.shift0)           \
        }                                                                      \
    } while (0)
    if (CAT) WINO_SET_SOURCE(chunk0 >= cp.c0Chunks);

    // Staging.  U slab: LDS-DMA (global_load_lds_dwordx4: a wave copies 64 consecutive float4 = 1 KiB per instruction straight into the slab,
    // no staging registers and -- what the ablation builds showed to matter -- no VGPR -> LDS store traffic: the four ds_write_b128 per thread
    // and chunk it replaces cost the kernel 20 %).  Activations: R quads per thread through registers (zero fill outside the image, split into
    // the channel-pair planes); plain scalars: arrays captured by reference went to scratch.
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 sxa = zero4, sxb = zero4, sxc = zero4, sxd = zero4;
    typedef __attribute__((address_space(3))) void* lds_ptr;
#define WINO_STAGE_LOAD(chunk_, buf_)                                                                                             \
    do {                                                                                                                          \
        const float4* u_ = uptr + static_cast<size_t>((chunk_) - chunk0) * UQ;                                                    \
        float* ub_ = (buf_) + 4 * (wave * 64);                                                                                    \
        if (!(SNNHIP_WINO_ABL & 64)) {                                                                                            \
            lds_dma16(u_, ub_);                                                                                                   \
            lds_dma16(u_ + NT, ub_ + 4 * NT);                                                                                     \
            lds_dma16(u_ + 2 * NT, ub_ + 8 * NT);                                                                                 \
            lds_dma16(u_ + 3 * NT, ub_ + 12 * NT);                                                                                \
        }                                                                                                                         \
        sxa = sxb = sxc = sxd = zero4;                                                                                            \
        if (SNNHIP_WINO_ABL & 128) break;                                                                                         \
        if (gofs[0] >= 0) sxa = *reinterpret_cast<const float4*>(CAT ? xs + gofs[0] + ((chunk_) - chunkOrg) * 8 : x + gofs[0] + (chunk_) * 8);                                     \
        if (gofs[1] >= 0) sxb = *reinterpret_cast<const float4*>(CAT ? xs + gofs[1] + ((chunk_) - chunkOrg) * 8 : x + gofs[1] + (chunk_) * 8);                                     \
        if (R > 2 && gofs[2] >= 0) sxc = *reinterpret_cast<const float4*>(CAT ? xs + gofs[2] + ((chunk_) - chunkOrg) * 8 : x + gofs[2] + (chunk_) * 8);                            \
        if (R > 2 && gofs[3] >= 0) sxd = *reinterpret_cast<const float4*>(CAT ? xs + gofs[3] + ((chunk_) - chunkOrg) * 8 : x + gofs[3] + (chunk_) * 8);                            \
    } while (0)
#define WINO_STORE_X(r_, v_)                                                                                     \
    if (lofs[r_] >= 0) {                                                                                         \
        *reinterpret_cast<float2*>(b_ + lofs[r_]) = make_float2(v_.x, v_.y);                                     \
        *reinterpret_cast<float2*>(b_ + lofs[r_] + p.planeStride) = make_float2(v_.z, v_.w);                     \
    }
#define WINO_STAGE_STORE(buf_)                                                                                   \
    do {                                                                                                         \
        float* b_ = (buf_);                                                                                      \
        WINO_STORE_X(0, sxa)                                                                                     \
        WINO_STORE_X(1, sxb)                                                                                     \
        if (R > 2) {                                                                                             \
            WINO_STORE_X(2, sxc)                                                                                 \
            WINO_STORE_X(3, sxd)                                                                                 \
        }                                                                                                        \
    } while (0)

    // ---- this lane's tile: t = 16 tg + n16 -> (image b, tile row, tile column) of the block tile
    const int t = 16 * tg + n16;
    const int ttx = t & (TTW - 1), tty = (t >> p.TTWs) & (TTH - 1), tbi = t >> (p.TTWs + p.TTHs);
    const int patch = kUFloats + k * p.planeStride + ((tbi * p.inH + 2 * tty) * p.rowPitch + 2 * ttx) * 2; // + (dy*rowPitch + dx)*2
    const int uoff = op * 256 + lane * 4;                                                                  // + pos * 256 * OPB: float4 {U[2op].s0, .s1, U[2op+1].s0, .s1}

    f32x4 acc[16][2];
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int o = 0; o < 2; ++o) acc[i][o] = f32x4{0.f, 0.f, 0.f, 0.f};

    WINO_STAGE_LOAD(chunk0, smem);
    WINO_STAGE_STORE(smem);
    lds_dma_wait();
    __syncthreads();

    for (int chunk = chunk0; chunk < chunk1; ++chunk) {
        const float* buf = smem + ((chunk - chunk0) & 1) * p.bufFloats;
        const bool more = chunk + 1 < chunk1;
        float* nbuf = smem + ((chunk + 1 - chunk0) & 1) * p.bufFloats; // the buffer nobody reads during this chunk
        if (CAT && chunk + 1 == cp.c0Chunks && more) WINO_SET_SOURCE(true); // (block-uniform, once per K range at the most)
        if (more && !(SNNHIP_WINO_ABL & 4)) WINO_STAGE_LOAD(chunk + 1, nbuf);

        // Issue order is pinned with sched_barrier: the patch and the first eight U operands are requested up front, the rest while the
        // first MFMAs run, and the next chunk goes to the OTHER LDS buffer in the middle of the MFMA stream (its global loads were issued a
        // thousand cycles earlier), so that the end of the chunk is only the barrier.  Left to itself the scheduler sinks every ds_read next
        // to its use (fewest registers) and the wave eats one LDS latency per position: 31 % matrix-pipe utilisation (PMC), 48 % after.
        float4 t4[4][2], u[16];
#define WINO_LDU(i) u[i] = (SNNHIP_WINO_ABL & 16) ? make_float4(1.f, 2.f, 3.f, 4.f) : *reinterpret_cast<const float4*>(buf + uoff + (i) * (256 * OPB))
#pragma unroll
        for (int dy = 0; dy < 4; ++dy)
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) // one ds_read_b128 = two adjacent pixels of the pair plane
                t4[dy][h2] = (SNNHIP_WINO_ABL & 32) ? make_float4(1.f + dy, 2.f, 3.f + h2, 4.f) : *reinterpret_cast<const float4*>(buf + patch + (dy * p.rowPitch + 2 * h2) * 2);
        WINO_LDU(0); WINO_LDU(1); WINO_LDU(2); WINO_LDU(3); WINO_LDU(4); WINO_LDU(5); WINO_LDU(6); WINO_LDU(7);
        __builtin_amdgcn_sched_barrier(0);
        // the 4x4 patch of (tile, channel pair), both channels of the pair
        float2 d[4][4];
#pragma unroll
        for (int dy = 0; dy < 4; ++dy)
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                d[dy][2 * h2] = make_float2(t4[dy][h2].x, t4[dy][h2].y);
                d[dy][2 * h2 + 1] = make_float2(t4[dy][h2].z, t4[dy][h2].w);
            }
        // V = Bt d B, Bt = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]
        float2 v[4][4];
#pragma unroll
        for (int j = 0; j < 4 && !(SNNHIP_WINO_ABL & 8); ++j) {
            const float2 a0 = d[0][j], a1 = d[1][j], a2 = d[2][j], a3 = d[3][j];
            d[0][j] = make_float2(a0.x - a2.x, a0.y - a2.y);
            d[1][j] = make_float2(a1.x + a2.x, a1.y + a2.y);
            d[2][j] = make_float2(a2.x - a1.x, a2.y - a1.y);
            d[3][j] = make_float2(a1.x - a3.x, a1.y - a3.y);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float2 a0 = d[i][0], a1 = d[i][1], a2 = d[i][2], a3 = d[i][3];
            if (SNNHIP_WINO_ABL & 8) {
                v[i][0] = a0; v[i][1] = a1; v[i][2] = a2; v[i][3] = a3;
                continue;
            }
            v[i][0] = make_float2(a0.x - a2.x, a0.y - a2.y);
            v[i][1] = make_float2(a1.x + a2.x, a1.y + a2.y);
            v[i][2] = make_float2(a2.x - a1.x, a2.y - a1.y);
            v[i][3] = make_float2(a1.x - a3.x, a1.y - a3.y);
        }
        // 16 positions x 2 channel blocks x 2 K steps: M[pos][oc][tile] += U[pos][oc][ic] V[pos][ic][tile]
#define WINO_STEP(pos)                                                                                       \
    do {                                                                                                     \
        const float2 vv_ = v[(pos) >> 2][(pos) & 3];                                                         \
        acc[pos][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(u[pos].x, vv_.x, acc[pos][0], 0, 0, 0);           \
        acc[pos][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(u[pos].z, vv_.x, acc[pos][1], 0, 0, 0);           \
        acc[pos][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(u[pos].y, vv_.y, acc[pos][0], 0, 0, 0);           \
        acc[pos][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(u[pos].w, vv_.y, acc[pos][1], 0, 0, 0);           \
    } while (0)
        WINO_STEP(0); WINO_STEP(1); WINO_STEP(2); WINO_STEP(3);
        __builtin_amdgcn_sched_barrier(0);
        WINO_LDU(8); WINO_LDU(9); WINO_LDU(10); WINO_LDU(11);
        __builtin_amdgcn_sched_barrier(0);
        WINO_STEP(4); WINO_STEP(5); WINO_STEP(6); WINO_STEP(7);
        __builtin_amdgcn_sched_barrier(0);
        WINO_LDU(12); WINO_LDU(13); WINO_LDU(14); WINO_LDU(15);
        if (more && !(SNNHIP_WINO_ABL & 2)) WINO_STAGE_STORE(nbuf);
        __builtin_amdgcn_sched_barrier(0);
        WINO_STEP(8); WINO_STEP(9); WINO_STEP(10); WINO_STEP(11); WINO_STEP(12); WINO_STEP(13); WINO_STEP(14); WINO_STEP(15);
#undef WINO_STEP
#undef WINO_LDU
        lds_dma_wait(); // (free here: the activation loads issued after the DMA were waited for by the stage store above)
        if (!(SNNHIP_WINO_ABL & 1)) __syncthreads();
    }

    // ---- KS = 2: the two K groups exchange one channel block's sums (region of wave w: [pos][lane] float4 = 16 KB, 128 KB in all; the staging buffers are
    // free: every wave is past the loop's last barrier)
    if (KS > 1) {
        f32x4* const xb = reinterpret_cast<f32x4*>(smemAll);
        f32x4* const mine = xb + ((ks * 4 + wave) * 16) * 64 + lane;
        const f32x4* const theirs = xb + (((1 - ks) * 4 + wave) * 16) * 64 + lane;
        if (ks == 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) mine[i * 64] = acc[i][1];
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) mine[i * 64] = acc[i][0];
        }
        __syncthreads();
        if (ks == 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i][0] += theirs[i * 64]; // p0 + p1
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i][1] = theirs[i * 64] + acc[i][1]; // p0 + p1 as well
        }
    }

    // ---- Y = At M A, At = [1 1 1 0; 0 1 -1 -1]; lane holds output channels 4k..4k+3 of each 16-channel block for its tile
    const int oy = oy0 + 2 * tty, ox = ox0 + 2 * ttx, n = b0 + tbi;
    const bool addSimple = act_is_simple_dev(p.ac2.act);
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        if (KS > 1 && o != ks) continue; // (wave-uniform: group g finishes channel block g)
        const int oc = blockIdx.y * (32 * OPB) + (2 * op + o) * 16 + 4 * k;
        if (oc >= p.OC) continue;
        // the epilogue rows of the lane's four channels and the residual of its 2 x 2 output pixels are requested FIRST, the inverse transform runs in
        // the shadow of those loads (requested where they are used -- a table load, then per pixel a residual load, each waited out -- they were eight
        // exposed L2 round trips per wave: conv1x1_stream's phase trace, DESIGN.md 5.1-8, found the same pattern)
        float4 e4[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) e4[c] = epi[oc + c];
        size_t idx4[2][2];
        bool ok4[2][2];
        float4 rv4[2][2];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int cx = 0; cx < 2; ++cx) {
                ok4[r][cx] = !(n >= p.N || oy + r >= p.OH || ox + cx >= p.OW);
                idx4[r][cx] = ((static_cast<size_t>(n) * p.OH + oy + r) * p.OW + ox + cx) * p.OC + oc;
                rv4[r][cx] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (!POOL && p.res && p.splitK == 1 && ok4[r][cx]) rv4[r][cx] = *reinterpret_cast<const float4*>(p.res + idx4[r][cx]);
            }
        f32x4 yv[2][2];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float t0[4], t1[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                t0[j] = acc[0 * 4 + j][o][c] + acc[1 * 4 + j][o][c] + acc[2 * 4 + j][o][c];
                t1[j] = acc[1 * 4 + j][o][c] - acc[2 * 4 + j][o][c] - acc[3 * 4 + j][o][c];
            }
            yv[0][0][c] = t0[0] + t0[1] + t0[2];
            yv[0][1][c] = t0[1] - t0[2] - t0[3];
            yv[1][0][c] = t1[0] + t1[1] + t1[2];
            yv[1][1][c] = t1[1] - t1[2] - t1[3];
        }
        // POOL (chain rule L): the tile origin is even in both directions, so yv[2][2] is exactly one 2x2 stride-2 pooling window.  bias -> BN -> activation on
        // each of its four values (BN's scale may be negative: the maximum stays behind it), then the pooling plan's own rule (eltwise_pool.hip): m = -100000,
        // m = max(m, v) over the positions inside the convolution's OH x OW (a window on the bottom / right edge is clipped; with the floor extent it is not
        // stored at all) -- ONE float4 per lane and channel block, no exchange, no LDS.  Split over blockIdx.z: raw partial tiles at full resolution below, as
        // ever; splitk_reduce_pool_kernel (conv2d_mfma.hip) sums, finishes and pools them.
        if (POOL && p.splitK == 1) {
            const int qy = oy >> 1, qx = ox >> 1;
            if (!ok4[0][0] || qy >= pq.poolOH || qx >= pq.poolOW) continue;
            float m4[4] = {-100000.0f, -100000.0f, -100000.0f, -100000.0f};
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int cx = 0; cx < 2; ++cx) {
                    if (!ok4[r][cx]) continue;
#pragma unroll
                    for (int c = 0; c < 4; ++c) m4[c] = fmaxf(m4[c], apply_act<SIMPLE>(ac, epi_affine(yv[r][cx][c], e4[c], p.useBN), 0.0f));
                }
            *reinterpret_cast<float4*>(y + ((static_cast<size_t>(n) * pq.poolOH + qy) * pq.poolOW + qx) * p.OC + oc) = make_float4(m4[0], m4[1], m4[2], m4[3]);
            continue;
        }
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int cx = 0; cx < 2; ++cx) {
                if (!ok4[r][cx]) continue;
                const size_t idx = idx4[r][cx];
                float o4[4];
                if (p.splitK > 1) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) o4[c] = yv[r][cx][c];
                    *reinterpret_cast<float4*>(ws + static_cast<size_t>(blockIdx.z) * (static_cast<size_t>(p.N) * p.OH * p.OW * p.OC) + idx) =
                        make_float4(o4[0], o4[1], o4[2], o4[3]);
                    continue;
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float vv = epi_affine(yv[r][cx][c], e4[c], p.useBN);
                    o4[c] = apply_act<SIMPLE>(ac, vv, 0.0f);
                }
                if (!POOL && p.res) {
                    const float4 rv = rv4[r][cx];
                    o4[0] = add_act(p.ac2, addSimple, o4[0] + rv.x);
                    o4[1] = add_act(p.ac2, addSimple, o4[1] + rv.y);
                    o4[2] = add_act(p.ac2, addSimple, o4[2] + rv.z);
                    o4[3] = add_act(p.ac2, addSimple, o4[3] + rv.w);
                }
                *reinterpret_cast<float4*>(y + idx) = make_float4(o4[0], o4[1], o4[2], o4[3]);
            }
    }
#undef WINO_SET_SOURCE
#undef WINO_DESCRIPTORS
#undef WINO_STAGE_LOAD
#undef WINO_STORE_X
#undef WINO_STAGE_STORE
