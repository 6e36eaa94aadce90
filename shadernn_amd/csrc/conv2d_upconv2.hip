// conv2d_upconv2.hip -- the "up-convolution" of the U-Net decoder: nearest x2 UpSampling2D -> Conv2D 2x2 stride 1 "same" (zero padding, one pad row
// and one pad column in total), fp32 and fp16, evaluated on the LOW-RESOLUTION tensor.  DESIGN.md section 4.30.
//
// Rule D on conv2d_mfma resolves the upsampling in its staging addresses and still multiplies 4 IC products per output pixel.  But along one axis, with
// pad offset p (0 or 1) in front, output coordinate 2 m + phase reads upsampled samples 2 m + phase - p + t, t = 0, 1, i.e. low-resolution samples
// m + floor((phase - p + t) / 2): the "double" phase D = 1 - p reads the two neighbours m - p and m - p + 1 (one tap each), the "single" phase S = p reads
// m twice (both taps).  In two dimensions the 2x2 output block of low-resolution pixel (m, q) needs (2 + 1) x (2 + 1) = 9 (phase, low-resolution pixel)
// products instead of 16, with the taps that fall on the same pixel ADDED UP beforehand (upconv2_presum, conv2d_upconv2.h; snnhip_upconv2_presum_weights):
//     out[2 m + py][2 q + px][oc] = sum over the entries (ey, ex) of phase (py, px), sum_ic  Wsum[ey][ex][oc][ic] * L[m - pr + a(ey)][q - pc + a(ex)][ic]
// with L zero outside the image (a low-resolution sample outside stands for two upsampled samples that are both outside: no partial case).
//
// Canonical form, so that one kernel serves both pad placements of either axis with static register indices: per axis the halo offset a' = 0 is the
// sample BOTH phases read (low-resolution index m: a = p), a' = 1 the one only D reads (a = 1 - p: m - 1 for p = 1, m + 1 for p = 0); the three entries
// are c = 0: (D, a' = 0), 1: (D, a' = 1), 2: (S, a' = 0).  p only moves the halo (run-time, wave-uniform) and names the output rows at the store.
//
//   block = 256 threads = 4 waves = a tile of kUpconv2TH x kUpconv2TW = 8 x 16 low-resolution pixels of one image (16 x 32 output pixels) x 16 NB channels
//   wave  = 2 tile rows (G = 2 pixel groups of 16 = the MFMA's N) x NB 16-channel row blocks (M), ALL FOUR phases: 4 accumulator sets of G x NB tiles.
//           Each of the four operand reads X[m + a'y][q + a'x] of a K chunk feeds every phase that uses the offset: 4 + 2 + 2 + 1 = 9 MFMA groups per 4 reads
//           (wave = phase would leave the waves with 1, 2, 2 and 4 terms).
//   MFMA  = v_mfma_f32_16x16x4_f32 (four per 16-byte operand: exact fma chains, as conv2d_mfma) / v_mfma_f32_16x16x32_f16, fp32 accumulation.  No
//           accumulator adds more than kUpconv2Chain = 1152 terms in a row: deeper layers (4 IC > 1152) flush into a second set every 1152 / (4 ICC) chunks
//           (FLUSH instantiations, NB = 2 so that both sets fit the registers without scratch).
//   input = per K chunk of 64 bytes (ICC = 16 floats / 32 halfs) the (8 + 1) x (16 + 1) halo tile, 16-byte loads, zero outside; the next chunk is fetched
//           into registers while this one computes and written to the other LDS buffer behind it (one barrier per chunk).  LDS pixel = 64 B = four
//           16-byte slots, slot' = slot ^ (((col >> 2) & 1) << 1): the conflict-free map of deconv2d_mfma.hip (same lane geometry: lane = (px, kq)).
//   weights = the nine [OC][IC] matrices packed once into the A-operand image [channel chunk][K chunk][entry cy * 3 + cx][row block][lane] x 16 bytes: a
//           block streams 9 NB KB per K chunk linearly from L2 / HBM.  Row m of block b is channel 32 (b >> 1) + 8 (m >> 2) + 4 (b & 1) + (m & 3), so a
//           lane's accumulators of a block pair are eight consecutive channels and the 2x2 output block of a pixel leaves straight from the accumulator
//           layout as 16-byte channel-contiguous vectors (the four kq of a pixel side by side: 128 B fp32 / 64 B fp16 per pixel and block pair).
//   tails = ragged tiles are masked at the store (their halo reads zeros), srcH / srcW of 1 are ragged tiles, n is a block index.  32-bit element offsets.
#include "conv2d_upconv2.h"
#include "epilogue.h"
#include "snnhip_internal.h"

namespace snnhip {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int TH = kUpconv2TH, TW = kUpconv2TW, HR = TH + 1, HC = TW + 1;
constexpr int G = TH / 4;                        // tile rows of a wave
constexpr int SLOTS = HR * HC * 4;               // 16-byte slots of a staged chunk
constexpr int ROUNDS = (SLOTS + 255) / 256;      // staging rounds
static_assert(ROUNDS == 3 && G == 2, "the staging registers below are named for three rounds, the accumulators for two rows per wave");

struct Up2Args {
    int N, srcH, srcW, IC, OC, OH, OW;
    int tilesX, tilesY, ocChunks;
    int pr, pc;        // pad offset of the rows (ConvGeom::pady) / columns (padx): 0 | 1
    int nch;           // K chunks of 64 bytes
    int flushEvery;    // FLUSH: chunks between two flushes
    int useBN;
};

__device__ __forceinline__ int halo_slot(int slot, int col) { return slot ^ (((col >> 2) & 1) << 1); }

template <typename T, int NB, bool FLUSH>
__global__ __launch_bounds__(256) void conv2d_upconv2_kernel(Up2Args a, ActCfg ac, const T* __restrict__ x, const uint4* __restrict__ wimg,
                                                            const float4* __restrict__ epi, T* __restrict__ y) {
    constexpr int ICC = 64 / static_cast<int>(sizeof(T)); // channels of a K chunk
    constexpr bool F16 = sizeof(T) == 2;
    __shared__ uint4 smem[2][SLOTS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, px = lane & 15, kq = lane >> 4;
    int bx = blockIdx.x;
    const int occ = bx % a.ocChunks; // the channel chunks of one tile run side by side: all but the first stage their input from L2
    bx /= a.ocChunks;
    const int tx = bx % a.tilesX;
    bx /= a.tilesX;
    const int ty = bx % a.tilesY, n = bx / a.tilesY;
    const int m0 = ty * TH, q0 = tx * TW;

    // ---- staging map: slot idx = tid + 256 r -> (halo row, halo column, 16-byte slot); halo (hr, hc) is low-resolution pixel (m0 - pr + hr, q0 - pc + hc)
    int gofs[ROUNDS], lofs[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int idx = tid + 256 * r;
        const int pos = idx >> 2, slot = idx & 3, hr = pos / HC, hc = pos - hr * HC;
        const int iy = m0 - a.pr + hr, ix = q0 - a.pc + hc;
        lofs[r] = idx < SLOTS ? pos * 4 + halo_slot(slot, hc) : -1;
        gofs[r] = (idx < SLOTS && iy >= 0 && iy < a.srcH && ix >= 0 && ix < a.srcW) ? ((n * a.srcH + iy) * a.srcW + ix) * a.IC + slot * (ICC / 4) : -1;
    }
    uint4 s0, s1, s2; // (named: an array captured by the lambdas below can end up in scratch memory)
    auto load_one = [&](int r, int ch) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (gofs[r] >= 0) v = *reinterpret_cast<const uint4*>(x + gofs[r] + ch * ICC);
        return v;
    };
    auto stage_load = [&](int ch) {
        s0 = load_one(0, ch);
        s1 = load_one(1, ch);
        s2 = load_one(2, ch);
    };
    auto stage_store = [&](uint4* buf) {
        if (lofs[0] >= 0) buf[lofs[0]] = s0;
        if (lofs[1] >= 0) buf[lofs[1]] = s1;
        if (lofs[2] >= 0) buf[lofs[2]] = s2;
    };

    // ---- operand addressing: lane (px, kq) reads slot kq of tile pixel (row0 + g, px) shifted by the canonical offset (a'y, a'x)
    const int row0 = wave * G;
    int colOf[2], rowOf[2], bofs[2][2];
    colOf[0] = px + a.pc; colOf[1] = px + 1 - a.pc; // a' = 0: the pixel itself (a = p), a' = 1: the neighbour only the double phase reads (a = 1 - p)
    rowOf[0] = row0 + a.pr; rowOf[1] = row0 + 1 - a.pr;
#pragma unroll
    for (int ay = 0; ay < 2; ++ay)
#pragma unroll
        for (int ax = 0; ax < 2; ++ax) bofs[ay][ax] = (rowOf[ay] * HC + colOf[ax]) * 4 + halo_slot(kq, colOf[ax]);

    // acc[dy][dx][g][nb]: d = 0 the double phase (output 2 m + 1 - p), d = 1 the single phase (2 m + p)
    f32x4 acc[2][2][G][NB], tot[FLUSH ? 2 : 1][FLUSH ? 2 : 1][FLUSH ? G : 1][FLUSH ? NB : 1];
#pragma unroll
    for (int i = 0; i < 4 * G * NB; ++i) (&acc[0][0][0][0])[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (FLUSH) {
#pragma unroll
        for (int i = 0; i < 4 * G * NB; ++i) (&tot[0][0][0][0])[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }

    // one weight operand x the G pixel groups of one offset -> the accumulators of one phase
    auto mfma_group = [&](const uint4 (&av)[NB], const uint4 (&bv)[G], f32x4 (&d)[G][NB]) {
        if constexpr (F16) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int g = 0; g < G; ++g)
                    d[g][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, av[nb]), __builtin_bit_cast(f16x8, bv[g]), d[g][nb], 0, 0, 0);
        } else { // component j outermost: G NB independent chains between two MFMAs on the same accumulator
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int g = 0; g < G; ++g)
                    d[g][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, av[nb].x), __builtin_bit_cast(float, bv[g].x), d[g][nb], 0, 0, 0);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int g = 0; g < G; ++g)
                    d[g][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, av[nb].y), __builtin_bit_cast(float, bv[g].y), d[g][nb], 0, 0, 0);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int g = 0; g < G; ++g)
                    d[g][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, av[nb].z), __builtin_bit_cast(float, bv[g].z), d[g][nb], 0, 0, 0);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int g = 0; g < G; ++g)
                    d[g][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, av[nb].w), __builtin_bit_cast(float, bv[g].w), d[g][nb], 0, 0, 0);
        }
    };

    const uint4* wch = wimg + static_cast<size_t>(occ) * a.nch * (9 * NB * 64) + lane; // this block's stream: [K chunk][entry][row block][lane]
    stage_load(0);
    stage_store(smem[0]);
    __syncthreads();
    int sinceFlush = 0;
    for (int ch = 0; ch < a.nch; ++ch) {
        const uint4* cur = smem[ch & 1];
        const bool more = ch + 1 < a.nch;
        if (more) stage_load(ch + 1);
#pragma unroll
        for (int ay = 0; ay < 2; ++ay)
#pragma unroll
            for (int ax = 0; ax < 2; ++ax) {
                uint4 bv[G];
#pragma unroll
                for (int g = 0; g < G; ++g) bv[g] = cur[bofs[ay][ax] + g * HC * 4];
                // offset (a'y, a'x) feeds phase (dy, dx) through entry (cy, cx), c = 0: (D, a' = 0), 1: (D, a' = 1), 2: (S, a' = 0)
#pragma unroll
                for (int dy = 0; dy < (ay ? 1 : 2); ++dy)
#pragma unroll
                    for (int dx = 0; dx < (ax ? 1 : 2); ++dx) {
                        const int cy = dy ? 2 : ay, cx = dx ? 2 : ax;
                        uint4 av[NB];
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb) av[nb] = wch[((cy * 3 + cx) * NB + nb) * 64];
                        mfma_group(av, bv, acc[dy][dx]);
                    }
            }
        wch += 9 * NB * 64;
        if constexpr (FLUSH) {
            if (++sinceFlush == a.flushEvery) { // (uniform) the chain of every accumulator ends here: kUpconv2Chain terms at the most
                sinceFlush = 0;
#pragma unroll
                for (int i = 0; i < 4 * G * NB; ++i) {
                    (&tot[0][0][0][0])[i] += (&acc[0][0][0][0])[i];
                    (&acc[0][0][0][0])[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                }
            }
        }
        if (more) stage_store(smem[(ch + 1) & 1]);
        __syncthreads();
    }
    if constexpr (FLUSH) {
#pragma unroll
        for (int i = 0; i < 4 * G * NB; ++i) (&acc[0][0][0][0])[i] += (&tot[0][0][0][0])[i];
    }

    // ---- epilogue: lane (px, kq) holds channels 16 (occ NB + nb) + 8 kq .. + 7 of a block pair (nb, nb + 1) at pixel (row0 + g, px), all four phases
    const bool simple = act_is_simple_dev(ac.act);
    const int q = q0 + px;
#pragma unroll
    for (int nb = 0; nb < NB; nb += 2) {
        const int oc = 16 * (occ * NB + nb) + 8 * kq;
        float4 e8[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) e8[i] = epi[oc + i];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx)
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int m = m0 + row0 + g;
                    if (m < a.srcH && q < a.srcW) {
                        const int oy = 2 * m + (dy ? a.pr : 1 - a.pr), ox = 2 * q + (dx ? a.pc : 1 - a.pc);
                        float o8[8];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float lo = epi_affine(acc[dy][dx][g][nb][i], e8[i], a.useBN), hi = epi_affine(acc[dy][dx][g][nb + 1][i], e8[4 + i], a.useBN);
                            o8[i] = simple ? apply_act<true>(ac, lo, 0.0f) : epi_act(ac.act, ac.leaky, lo, 0.0f);
                            o8[4 + i] = simple ? apply_act<true>(ac, hi, 0.0f) : epi_act(ac.act, ac.leaky, hi, 0.0f);
                        }
                        T* dst = y + ((n * a.OH + oy) * a.OW + ox) * a.OC + oc;
                        if constexpr (F16) {
                            stv<T, 8>(dst, o8);
                        } else {
                            const float lo4[4] = {o8[0], o8[1], o8[2], o8[3]}, hi4[4] = {o8[4], o8[5], o8[6], o8[7]};
                            stv<T, 4>(dst, lo4);
                            stv<T, 4>(dst + 4, hi4);
                        }
                    }
                }
    }
}

typedef void (*Up2Kernel32)(Up2Args, ActCfg, const float*, const uint4*, const float4*, float*);
typedef void (*Up2Kernel16)(Up2Args, ActCfg, const _Float16*, const uint4*, const float4*, _Float16*);

struct Upconv2Plan : ConvPlanBase {
    Up2Args a;
    ActCfg ac;
    float* d_w = nullptr;
    float* d_epi = nullptr;
    int NB = 2;
    bool flush = false;
    dim3 grid;

    template <typename T>
    int launch(const snnhip_tensor* x, snnhip_tensor* out) {
        const T* xp = reinterpret_cast<const T*>(x->data);
        T* yp = reinterpret_cast<T*>(out->data);
        const uint4* w = reinterpret_cast<const uint4*>(d_w);
        const float4* e = reinterpret_cast<const float4*>(d_epi);
        if (flush) SNNHIP_LAUNCH((conv2d_upconv2_kernel<T, 2, true>), grid, dim3(256), 0, ctx->stream, a, ac, xp, w, e, yp);
        else if (NB == 4) SNNHIP_LAUNCH((conv2d_upconv2_kernel<T, 4, false>), grid, dim3(256), 0, ctx->stream, a, ac, xp, w, e, yp);
        else SNNHIP_LAUNCH((conv2d_upconv2_kernel<T, 2, false>), grid, dim3(256), 0, ctx->stream, a, ac, xp, w, e, yp);
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }

    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        SNNHIP_REQUIRE(nIn == 1, "conv2d: expects 1 input, got %d", nIn);
        const snnhip_tensor* x = in[0];
        SNNHIP_REQUIRE(x->n == a.N && x->h == a.srcH && x->w == a.srcW && x->c == a.IC, "conv2d: input dims %dx%dx%dx%d != plan %dx%dx%dx%d", x->n, x->h, x->w,
                       x->c, a.N, a.srcH, a.srcW, a.IC);
        SNNHIP_REQUIRE(out->n == a.N && out->h == a.OH && out->w == a.OW && out->c == a.OC, "conv2d: output dims %dx%dx%dx%d != plan %dx%dx%dx%d", out->n,
                       out->h, out->w, out->c, a.N, a.OH, a.OW, a.OC);
        SNNHIP_REQUIRE(x->dtype == dtype && out->dtype == dtype, "conv2d_upconv2: tensor dtypes %d -> %d, the plan's is %d", x->dtype, out->dtype, dtype);
        return dtype == SNNHIP_F16 ? launch<_Float16>(x, out) : launch<float>(x, out);
    }
};

} // namespace

// the layer's shape alone (no context): what snnhip_upconv2_presum_weights and the plan both require of the convolution itself
static bool upconv2_layer_ok(int kh, int kw, int sh, int sw, int padMode) {
    return kh == 2 && kw == 2 && sh == 1 && sw == 1 && padMode == SNNHIP_PAD_CONSTANT;
}

// Default routing, per (precision, shape class: the shallow layers on 128 accumulators, the deep ones with the flush), from the alternated measurement of
// tools/bench_upconv2.py against the direct kernel in the same process (profiles/upconv2_layers.json): a class is taken where it won by more than the
// run's own spread.  SNNHIP_CONV=upconv2 takes every eligible layer.
// Measured at batch 8: fp32 1.05x .. 1.62x faster on all four U-Net layers, both classes; fp16 0.45x .. 0.60x (its MFMAs are eight times shorter per 16-byte
// weight operand: the weight stream from L2 bounds it), so fp16 stays on the direct kernel unless forced.
static bool upconv2_default(bool f16, bool flush) {
    (void) flush;
    return !f16;
}

// Tried by make_conv2d_mfma_plan (conv2d_mfma.hip) in front of the direct kernel; SNNHIP_E_UNSUPPORTED hands the layer on.
int make_conv2d_upconv2_plan(snnhip_ctx* ctx, const ConvGeom& g, const float* w_oihw, const std::vector<float>& epi4, snnhip_plan** out) {
    const bool f16 = g.dtype == SNNHIP_F16;
    const char* force = snnhip::option("SNNHIP_CONV");
    const bool forced = force && strcmp(force, "upconv2") == 0;
    if (g.preShift != 1 || g.preMode != SNNHIP_PAD_CONSTANT || g.preX != 0 || g.preY != 0 || !upconv2_layer_ok(g.kh, g.kw, g.sh, g.sw, g.padMode)) return SNNHIP_E_UNSUPPORTED;
    if (g.dtype != SNNHIP_F32 && !f16) return SNNHIP_E_UNSUPPORTED;
    // one pad row and one pad column in total, on either side: the output is the upsampled extent and the near pads are 0 or 1
    if (g.padx < 0 || g.padx > 1 || g.pady < 0 || g.pady > 1 || g.H != 2 * g.srcH || g.W != 2 * g.srcW || g.OH != g.H || g.OW != g.W) return SNNHIP_E_UNSUPPORTED;
    if (g.addAct >= 0 || g.normShift || g.act == SNNHIP_ACT_SILU_QUIRK) return SNNHIP_E_UNSUPPORTED; // rules E and I, the 4-pixel quirk: the direct kernel's
    const int ICC = kUpconv2ICBytes / (f16 ? 2 : 4);
    if (g.IC % ICC != 0 || g.OC % kUpconv2OC != 0) {
        set_error("conv2d_upconv2: ic=%d oc=%d: the kernel takes IC in multiples of %d (%d bytes) and OC in multiples of %d", g.IC, g.OC, ICC, kUpconv2ICBytes, kUpconv2OC);
        return SNNHIP_E_UNSUPPORTED;
    }
    if (static_cast<double>(g.N) * g.srcH * g.srcW * g.IC >= 2147483647.0 || static_cast<double>(g.N) * g.OH * g.OW * g.OC >= 2147483647.0) return SNNHIP_E_UNSUPPORTED; // 32-bit element offsets
    Up2Args a = {};
    a.N = g.N; a.srcH = g.srcH; a.srcW = g.srcW; a.IC = g.IC; a.OC = g.OC; a.OH = g.OH; a.OW = g.OW;
    a.pr = g.pady; a.pc = g.padx; // sic: rows are offset by padL, columns by padT (ConvGeom)
    a.tilesX = up_div(g.srcW, TW); a.tilesY = up_div(g.srcH, TH);
    a.nch = g.IC / ICC;
    a.useBN = g.useBN;
    const bool flush = 4 * g.IC > kUpconv2Chain;
    const int NB = (!flush && g.OC % 64 == 0) ? 4 : 2;
    a.flushEvery = flush ? kUpconv2Chain / (4 * ICC) : 0;
    a.ocChunks = g.OC / (16 * NB);
    if (static_cast<double>(a.tilesX) * a.tilesY * g.N * a.ocChunks >= 2147483647.0) return SNNHIP_E_UNSUPPORTED;
    if (!forced && !upconv2_default(f16, flush)) return SNNHIP_E_UNSUPPORTED;

    auto* plan = new Upconv2Plan();
    plan->ctx = ctx;
    plan->g = g;
    plan->w_oihw.assign(w_oihw, w_oihw + static_cast<size_t>(g.OC) * g.IC * 4);
    plan->epi4 = epi4;
    plan->a = a;
    plan->ac = make_act_cfg(g.act, g.leaky);
    plan->NB = NB;
    plan->flush = flush;
    plan->grid = dim3(static_cast<unsigned>(a.tilesX) * a.tilesY * g.N * a.ocChunks);
    plan->dtype = g.dtype;

    // the nine matrices in the documented order (fp16: of the half-rounded taps, the sum rounded to half once, as conv2d_upconv does) ...
    const size_t mat = static_cast<size_t>(g.OC) * g.IC;
    std::vector<float> sum9(9 * mat);
    if (f16) {
        std::vector<float> wh(4 * mat);
        for (size_t i = 0; i < wh.size(); ++i) wh[i] = static_cast<float>(static_cast<_Float16>(w_oihw[i]));
        upconv2_presum(wh.data(), g.OC, g.IC, a.pr, a.pc, sum9.data());
    } else {
        upconv2_presum(w_oihw, g.OC, g.IC, a.pr, a.pc, sum9.data());
    }
    // ... into the A-operand image [channel chunk][K chunk][canonical entry cy * 3 + cx][row block][lane] x 16 bytes.  Canonical c -> documented e:
    // c = 0 (double phase, the pixel itself) is e = 1 for either p; c = 1 (double phase, the neighbour) is e = 0 (p = 1) / 2 (p = 0); c = 2 (single phase) the other
    const int eOf[2][3] = {{1, 2, 0}, {1, 0, 2}};
    const int per = ICC / 4;
    std::vector<float> img(static_cast<size_t>(a.ocChunks) * a.nch * 9 * NB * 64 * 4, 0.0f);
    _Float16* imgh = reinterpret_cast<_Float16*>(img.data());
    size_t at = 0;
    for (int occ = 0; occ < a.ocChunks; ++occ)
        for (int ch = 0; ch < a.nch; ++ch)
            for (int c = 0; c < 9; ++c) {
                const float* src = sum9.data() + static_cast<size_t>(3 * eOf[a.pr][c / 3] + eOf[a.pc][c % 3]) * mat;
                for (int nb = 0; nb < NB; ++nb)
                    for (int lane = 0; lane < 64; ++lane, ++at) {
                        const int b = occ * NB + nb, m = lane & 15, kq = lane >> 4, oc = 32 * (b >> 1) + 8 * (m >> 2) + 4 * (b & 1) + (m & 3);
                        for (int j = 0; j < per; ++j) {
                            const float wv = src[static_cast<size_t>(oc) * g.IC + ch * ICC + kq * per + j];
                            if (f16) imgh[at * 8 + j] = static_cast<_Float16>(wv);
                            else img[at * 4 + j] = wv;
                        }
                    }
            }
    int rc = plan->upload(img.data(), img.size(), &plan->d_w);
    if (rc == SNNHIP_OK) rc = plan->upload(epi4.data(), epi4.size(), &plan->d_epi);
    if (rc != SNNHIP_OK) {
        delete plan;
        return rc;
    }
    plan->inDims[0] = g.N; plan->inDims[1] = g.srcH; plan->inDims[2] = g.srcW; plan->inDims[3] = g.IC;
    plan->outDims[0] = g.N; plan->outDims[1] = g.OH; plan->outDims[2] = g.OW; plan->outDims[3] = g.OC;
    plan->flops = 2.0 * 4 * g.IC * g.OC * static_cast<double>(g.OH) * g.OW * g.N; // the nominal count of the 2x2 layer; issued: 9 / 16 of it on whole tiles
    const double esz = f16 ? 2.0 : 4.0;
    plan->bytes = esz * (static_cast<double>(g.N) * g.srcH * g.srcW * g.IC + static_cast<double>(g.N) * g.OH * g.OW * g.OC + 9.0 * mat);
    char buf[400];
    snprintf(buf, sizeof(buf), "conv2d_mfma_upconv2_%s k=2x2 s=1 ic=%d oc=%d as 9 pre-summed (phase, low-res pixel) GEMMs, tile=%dx%d low-res px (%dx%d out) x %doc "
                               "chunk=%d pad=(%d,%d)%s lds=%zuB mfma_flops=%.6g +pad(constant) +upsample(x2)",
             f16 ? "f16_16x16x32" : "f32_16x16x4", g.IC, g.OC, TH, TW, 2 * TH, 2 * TW, 16 * NB, ICC, a.pr, a.pc, flush ? " flush=1152" : "", sizeof(uint4) * 2 * SLOTS,
             2.0 * 9 * g.IC * g.OC * static_cast<double>(a.tilesX) * a.tilesY * TH * TW * g.N);
    plan->desc = buf;
    *out = plan;
    return SNNHIP_OK;
}

} // namespace snnhip

// include/snnhip.h: the host-side statement of the pre-summation (no context, no device)
extern "C" int snnhip_upconv2_presum_weights(const snnhip_conv2d_desc* d, const float* w_oihw, float* out) {
    using namespace snnhip;
    SNNHIP_REQUIRE(d && w_oihw && out, "upconv2_presum_weights: null argument");
    SNNHIP_REQUIRE(d->IC > 0 && d->OC > 0, "upconv2_presum_weights: ic=%d oc=%d", d->IC, d->OC);
    SNNHIP_REQUIRE(upconv2_layer_ok(d->kh, d->kw, d->sh, d->sw, d->padMode), "upconv2_presum_weights: k=%dx%d s=%dx%d padMode=%d (a 2x2 stride-1 layer with constant padding)",
                   d->kh, d->kw, d->sh, d->sw, d->padMode);
    SNNHIP_REQUIRE(d->padT >= 0 && d->padB >= 0 && d->padL >= 0 && d->padR >= 0 && d->padT + d->padB == 1 && d->padL + d->padR == 1,
                   "upconv2_presum_weights: pads T=%d B=%d L=%d R=%d (one pad row and one pad column in total)", d->padT, d->padB, d->padL, d->padR);
    upconv2_presum(w_oihw, d->OC, d->IC, d->padL, d->padT, out); // sic: rows are offset by padL, columns by padT
    return SNNHIP_OK;
}
