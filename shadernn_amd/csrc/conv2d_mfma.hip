// conv2d_mfma.hip -- fp32 implicit-GEMM convolution on the gfx950 matrix cores (v_mfma_f32_32x32x2_f32) for the
// GEMM-shaped layers of the reference's Conv2D operator (3x3 / 1x1 / 7x7 ... with IC >= 8): ResNet-18 / MobileNetV2
// pointwise / Candy style convolutions (BASELINE configs[2..4]).
//
// Replaces shadertemplate_vk_conv2d.comp:148-347 and shadertemplate_vk_conv2d_1x1.comp:68-210 of the reference for those
// shapes; arithmetic, padding modes, epilogue (bias -> BN -> activation) and the SiLU 4-pixel quirk are the same as in
// conv2d_generic.hip, only the reduction order differs (fp32 accumulate in the MFMA).
//
// GEMM view:  M = output pixels, N = output channels, K = (tap, ic).
//   block  = 256 threads = 4 waves; block tile = 128 pixels x BN channels, BN in {32, 64, 128}
//   pixels of a block tile = TB images x TH rows x TW columns (TB*TH*TW = 128, picked per layer to fit OH x OW)
//   wave   = MT x NT MFMA tiles of 32 x 32 (16 fp32 accumulators per lane per tile)
//   A (activations): per 16-channel chunk (8 when IC <= 8) the input halo tile of the block is staged ONCE in LDS
//       lds[(b, row, col)][pitch = chunk + 4]          (pitch 20 / 12 floats: conflict-free ds_read_b128)
//     and re-used by all kh*kw taps: a tap is just a different LDS offset.  Next chunk's tile is fetched into registers
//     while the MFMAs of this chunk run and written to the other LDS buffer afterwards (one barrier per chunk).
//   B (weights): pre-packed on the host so that one lane reads ONE float4 per MFMA tile and K-step, straight from
//     global/L2 (the stream is purely linear over the K loop):
//       Wp[chunk][tap][c8][h][ocPadded][j],   ic = chunk*ICc + c8*8 + h*4 + j
//     The K order inside an 8-channel step is permuted (h = lane/32 owns channels 4h..4h+3, MFMA j consumes component
//     j) so that both operands of four consecutive MFMAs come from one 16-byte load.
//   D: lane l holds column (oc) l%32 and rows 8*(r/4) + 4*(l/32) + r%4 -> a store instruction writes 32 consecutive
//     channels of one pixel (128 B) per half-wave; the epilogue parameters are per-lane constants.
#include <mutex>

#include "conv2d_mfma_kernel.h"

namespace snnhip {

using namespace mfma_detail;

// one translation unit per block width and precision (conv2d_mfma_bn{128,64,32}_{f32,f16}.hip)
KernelFn pick_conv2d_mfma_bn128_f32(int c8, int r, bool simple, int taps);
KernelFn pick_conv2d_mfma_bn64_f32(int c8, int r, bool simple, int taps);
KernelFn pick_conv2d_mfma_bn32_f32(int c8, int r, bool simple, int taps);
KernelFn pick_conv2d_mfma_bn128_f16(int c8, int r, bool simple, int taps);
KernelFn pick_conv2d_mfma_bn64_f16(int c8, int r, bool simple, int taps);
KernelFn pick_conv2d_mfma_bn32_f16(int c8, int r, bool simple, int taps);

namespace {

template <bool SIMPLE, typename T>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(size_t MN, int OC, int splitK, int useBN, ActCfg ac, const float* __restrict__ ws,
                                                           const float4* __restrict__ epi, T* __restrict__ y, const T* __restrict__ res, ActCfg ac2) {
    const bool addSimple = act_is_simple_dev(ac2.act);
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < MN; i += static_cast<size_t>(gridDim.x) * 256) {
        float v = 0.0f;
        for (int z = 0; z < splitK; ++z) v += ws[static_cast<size_t>(z) * MN + i];
        v = epi_affine(v, epi[i % OC], useBN);
        v = SIMPLE ? apply_act<true>(ac, v, 0.0f) : epi_act(ac.act, ac.leaky, v, 0.0f);
        if (res) v = add_act(ac2, addSimple, v + static_cast<float>(res[i])); // fused residual Add: on the fp32 value, one rounding on store
        y[i] = static_cast<T>(v);
    }
}

// The same pass for fp32 tensors with OC % 4 == 0 and at most eight partial sums (every split-K layer of ResNet-18): a thread owns four consecutive
// channels of one pixel, ALL its partial-sum loads (and the residual's) are in flight before the first addition, and the channel of an element comes from
// one 32-bit division per thread instead of a 64-bit modulo per element.  The generic kernel above walks the partial sums one dependent load after the
// other -- Z L2 round trips per element and thread: 8 us for 1.6 M outputs, nine such launches per ResNet-18 inference.  Same summation order (z = 0 first).
template <bool SIMPLE>
__global__ __launch_bounds__(256) void splitk_reduce4_kernel(unsigned MN4, unsigned OC4, int splitK, int useBN, ActCfg ac, const float4* __restrict__ ws,
                                                            const float4* __restrict__ epi, float4* __restrict__ y, const float4* __restrict__ res, ActCfg ac2) {
    const bool addSimple = act_is_simple_dev(ac2.act);
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < MN4; i += gridDim.x * 256u) {
        float4 part[8];
#pragma unroll
        for (int z = 0; z < 8; ++z) part[z] = ws[static_cast<size_t>(min(z, splitK - 1)) * MN4 + i]; // (unconditional: a partly written register array goes to scratch)
        float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (res) rv = res[i];
        const unsigned c4 = (i % OC4) * 4u;
        const float4 e0 = epi[c4], e1 = epi[c4 + 1], e2 = epi[c4 + 2], e3 = epi[c4 + 3];
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int z = 0; z < 8; ++z)
            if (z < splitK) {
                v[0] += part[z].x;
                v[1] += part[z].y;
                v[2] += part[z].z;
                v[3] += part[z].w;
            }
        const float4 ee[4] = {e0, e1, e2, e3};
        const float rr[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float t = epi_affine(v[k], ee[k], useBN);
            t = SIMPLE ? apply_act<true>(ac, t, 0.0f) : epi_act(ac.act, ac.leaky, t, 0.0f);
            if (res) t = add_act(ac2, addSimple, t + rr[k]);
            v[k] = t;
        }
        y[i] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

} // namespace

// Launches the split-K reduce / epilogue pass: out = [act2(] act(BN(bias + sum_z ws[z])) [+ res)], shared with conv2d_wino.hip.
int launch_splitk_reduce(snnhip_ctx* ctx, int OC, int splitK, int useBN, const ActCfg& ac, const float* ws, const float4* e4, snnhip_tensor* out,
                         const snnhip_tensor* res, const ActCfg& ac2) {
    const size_t MN = out->count();
    size_t blocks = (MN + 255) / 256;
    const size_t cap = static_cast<size_t>(ctx->props.multiProcessorCount > 0 ? ctx->props.multiProcessorCount : 256) * 8;
    if (blocks > cap) blocks = cap;
    const dim3 gr(static_cast<unsigned>(blocks));
    const bool simple = act_is_simple(ac.act);
    if (out->dtype == SNNHIP_F16) {
        _Float16* yo = reinterpret_cast<_Float16*>(out->data);
        const _Float16* rr = res ? reinterpret_cast<const _Float16*>(res->data) : nullptr;
        if (simple) SNNHIP_LAUNCH((splitk_reduce_kernel<true, _Float16>), gr, dim3(256), 0, ctx->stream, MN, OC, splitK, useBN, ac, ws, e4, yo, rr, ac2);
        else SNNHIP_LAUNCH((splitk_reduce_kernel<false, _Float16>), gr, dim3(256), 0, ctx->stream, MN, OC, splitK, useBN, ac, ws, e4, yo, rr, ac2);
    } else if (OC % 4 == 0 && splitK <= 8 && MN / 4 < 0xffffffffull && !snnhip::option("SNNHIP_SPLITK_REDUCE_SCALAR")) {
        const unsigned MN4 = static_cast<unsigned>(MN / 4);
        const dim3 g4(static_cast<unsigned>(std::min<size_t>((MN4 + 255) / 256, cap)));
        const float4* rr = res ? reinterpret_cast<const float4*>(res->data) : nullptr;
        if (simple) SNNHIP_LAUNCH((splitk_reduce4_kernel<true>), g4, dim3(256), 0, ctx->stream, MN4, static_cast<unsigned>(OC / 4), splitK, useBN, ac, reinterpret_cast<const float4*>(ws), e4,
                                  reinterpret_cast<float4*>(out->data), rr, ac2);
        else SNNHIP_LAUNCH((splitk_reduce4_kernel<false>), g4, dim3(256), 0, ctx->stream, MN4, static_cast<unsigned>(OC / 4), splitK, useBN, ac, reinterpret_cast<const float4*>(ws), e4,
                           reinterpret_cast<float4*>(out->data), rr, ac2);
    } else {
        const float* rr = res ? res->data : nullptr;
        if (simple) SNNHIP_LAUNCH((splitk_reduce_kernel<true, float>), gr, dim3(256), 0, ctx->stream, MN, OC, splitK, useBN, ac, ws, e4, out->data, rr, ac2);
        else SNNHIP_LAUNCH((splitk_reduce_kernel<false, float>), gr, dim3(256), 0, ctx->stream, MN, OC, splitK, useBN, ac, ws, e4, out->data, rr, ac2);
    }
    SNNHIP_CHECK_HIP(hipGetLastError());
    return SNNHIP_OK;
}

namespace {

struct MfmaConvPlan : ConvPlanBase {
    float* d_ws = nullptr; // split-K workspace
    MfmaParams p;
    ActCfg ac;
    float* d_w = nullptr;
    float* d_epi = nullptr;
    size_t ldsBytes = 0;
    dim3 grid;
    void (*kernel)(MfmaParams, ActCfg, const void*, const void*, const float4*, void*, float*) = nullptr;

    bool fusedAdd = false; // chain rule E: run(x, residual) -> act2(conv(x) + residual)
    bool enableTileStats() override {
        if (statPart) return true;
        if (dtype != SNNHIP_F16 || !p.ldsEpi || p.splitK != 1 || p.TBs != 0 || fusedAdd) return false;
        const int BN = p.OCp / static_cast<int>(grid.y);
        const size_t need = std::max(static_cast<size_t>(128) * (BN + 8) * 2, static_cast<size_t>(2) * 256 * 8 * sizeof(float)); // output tile, then the fold scratch over it
        if (need > ldsBytes) {
            if (need > 64 * 1024 &&
                hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(need)) != hipSuccess)
                return false;
            ldsBytes = need;
        }
        void* buf = nullptr;
        const size_t bytes = static_cast<size_t>(p.N) * p.tilesY * p.tilesX * 2 * p.OC * sizeof(float);
        if (snnhip::dev_malloc(&buf, bytes) != hipSuccess) return false;
        deviceAllocs.push_back(buf);
        statPart = p.statPart = static_cast<float*>(buf);
        statTilesX = p.tilesX; statTilesY = p.tilesY; statTH = 1 << p.THs; statTW = 1 << p.TWs;
        desc += " +tile-stats";
        return true;
    }
    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        SNNHIP_REQUIRE(nIn == (fusedAdd ? 2 : 1), "conv2d: expects %d input(s), got %d", fusedAdd ? 2 : 1, nIn);
        const snnhip_tensor* x = in[0];
        MfmaParams p = this->p; // per-launch copy: the residual pointer travels in the kernel argument block
        p.res = nullptr;
        if (fusedAdd) {
            const snnhip_tensor* r = in[1];
            SNNHIP_REQUIRE(r->n == p.N && r->h == p.OH && r->w == p.OW && r->c == p.OC && r->dtype == dtype,
                           "conv2d+add: residual %dx%dx%dx%d (dtype %d) does not match the output %dx%dx%dx%d", r->n, r->h, r->w, r->c, r->dtype, p.N, p.OH,
                           p.OW, p.OC);
            p.res = p.splitK > 1 ? nullptr : static_cast<const void*>(r->data); // split-K: the reduce pass adds it
        }
        SNNHIP_REQUIRE(x->n == p.N && x->h == p.srcH && x->w == p.srcW && x->c == p.IC, "conv2d: input dims %dx%dx%dx%d != plan %dx%dx%dx%d",
                       x->n, x->h, x->w, x->c, p.N, p.srcH, p.srcW, p.IC);
        SNNHIP_REQUIRE(out->n == p.N && out->h == p.OH && out->w == p.OW && out->c == p.OC, "conv2d: output dims %dx%dx%dx%d != plan %dx%dx%dx%d",
                       out->n, out->h, out->w, out->c, p.N, p.OH, p.OW, p.OC);
        SNNHIP_LAUNCH(kernel, grid, dim3(256), ldsBytes, ctx->stream, p, ac, static_cast<const void*>(x->data), static_cast<const void*>(d_w),
                           reinterpret_cast<const float4*>(d_epi), static_cast<void*>(out->data), d_ws);
        if (p.splitK > 1)
            return launch_splitk_reduce(ctx, p.OC, p.splitK, p.useBN, ac, d_ws, reinterpret_cast<const float4*>(d_epi), out, fusedAdd ? in[1] : nullptr, p.ac2);
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }
};

} // namespace

namespace {
struct MfmaOverride {
    int bn = 0;     // 32 | 64 | 128, 0 = heuristic
    int splitK = 0; // >= 1, 0 = heuristic
};
} // namespace

static int make_conv2d_mfma_plan_ex(snnhip_ctx* ctx, const ConvGeom& g, const float* w_oihw, const std::vector<float>& epi4, const MfmaOverride& ov,
                                    snnhip_plan** out) {
    // routing: GEMM-shaped layers only (north star: "MFMA used only for the dense 3x3/1x1 GEMM-shaped convs");
    // SNNHIP_CONV=generic|mfma forces a path (tests exercise both on the same inputs)
    const char* force = snnhip::option("SNNHIP_CONV");
    if (force && strcmp(force, "generic") == 0) return SNNHIP_E_UNSUPPORTED;
    const bool forced = force && strcmp(force, "mfma") == 0;
    // measured (tools/bench_layers.py): even IC = 3 layers (one 8-channel chunk, 5/8 of it padding) run 1.4-2.3x faster here than
    // on the VALU kernel, so only the channel-thin outputs (OC < 16: most of a 32-wide MFMA column block would be padding) stay there
    // and the 16-wide thin layers (OC < 32 with IC < 32, e.g. ESPCN's 16->16: half of the narrowest 32-wide block is padding) measured
    // faster there too (241 vs 276 us at 1080p)
    const bool f16 = g.dtype == SNNHIP_F16; // fp16 tensors: this is the only general convolution kernel, it takes every shape
    if (!forced && !f16 && (g.OC < 16 || (g.OC < 32 && g.IC < 32))) return SNNHIP_E_UNSUPPORTED;
    const double inCount = static_cast<double>(g.N) * (g.preMode ? g.srcH : g.H) * (g.preMode ? g.srcW : g.W) * g.IC;
    const double outCount = static_cast<double>(g.N) * g.OH * g.OW * g.OC;
    if (inCount >= 2147483647.0 || outCount >= 2147483647.0) return SNNHIP_E_UNSUPPORTED; // 32-bit element offsets in the kernel

    // graph rule I (InstanceNorm applied in the staging): the fp16 kernels with whole 8-channel slots, one image per pixel tile
    const bool preNorm = g.normShift != nullptr;
    if (preNorm && (!f16 || g.IC % 8 != 0 || !act_is_simple(g.normAct))) return SNNHIP_E_UNSUPPORTED;

    const int taps = g.kh * g.kw;
    // channels per LDS chunk: 16 (8 when IC <= 8).  Wider chunks (the kernel is instantiated up to 64 channels; SNNHIP_CONV_C8=4|8 selects
    // them for pointwise stride-1 layers) were measured on the MobileNetV2 layers: fewer barriers per MFMA, but the 4x staging registers and
    // LDS cost more residency than they save (1x1 960->320 @7x7 b32: 58.7 -> 51.7 us, 144->24 @56x56: 27.9 -> 45.3 us), so 16 stays the default
    const int CH = f16 ? 8 : 4;                                  // channels per 16-byte slot
    int C8 = g.IC <= 2 * CH ? 1 : 2;
    // tap-pair mode (C8 = 0, see the kernel): channel-thin inputs with at least two taps; SNNHIP_CONV_PAIR=0 keeps the channel-chunk path
    const char* pairEnv = snnhip::option("SNNHIP_CONV_PAIR");
    if (g.IC <= CH && taps >= 2 && !(pairEnv && atoi(pairEnv) == 0) && !preNorm) C8 = 0;
    if (const char* e = snnhip::option("SNNHIP_CONV_C8"))
        if (taps == 1 && g.sh == 1 && g.sw == 1 && (atoi(e) == 4 || atoi(e) == 8) && g.IC >= 2 * CH * atoi(e)) C8 = atoi(e);
    int Qs = C8 ? 2 * C8 : 1;                                    // 16-byte slots per staged pixel
    int ICc = C8 ? 2 * CH * C8 : CH;                             // channels per LDS chunk: 16 fp32 / 32 fp16 (64 bytes per pixel either way)

    if (g.sw < 1 || g.sw > 2 || g.sh < 1 || g.sh > 2) return SNNHIP_E_UNSUPPORTED;

    // pixel tile: TB x TH x TW = 128, minimising padded pixels, then the staged halo
    struct TileLayout {
        int tileH, tileW, rowPitch, imgPitch, evenCols, total;
        size_t ldsBytes;
    };
    auto layout = [&](int TBs, int THs, int TWs) {
        const int TB = 1 << TBs, TH = 1 << THs, TW = 1 << TWs;
        TileLayout L;
        L.tileH = (TH - 1) * g.sh + g.kh;
        L.tileW = (TW - 1) * g.sw + g.kw;
        L.evenCols = g.sw == 2 ? (L.tileW + 1) / 2 : 0;
        L.rowPitch = L.tileW;
        if (TW < 32)  // lanes of one 32-lane half span several tile rows: their row step must be == TW (mod 16)
            while ((g.sh * L.rowPitch) % 16 != TW % 16) ++L.rowPitch;
        L.imgPitch = round_up(L.tileH * L.rowPitch, 16);
        L.total = TB * L.tileH * L.tileW * Qs;
        L.ldsBytes = static_cast<size_t>(2) * TB * L.imgPitch * Qs * 16;
        return L;
    };
    static const int shapes[][3] = {{0, 3, 4}, {0, 2, 5}, {0, 4, 3}, {1, 3, 3}, {2, 2, 3}, {3, 2, 2}, {0, 1, 6}, {0, 0, 7}};
    int best = -1;
    double bestCost = 0;
    size_t bestLds = 0;
    auto choose = [&]() {
        best = -1;
        const bool oneChunk = up_div(g.IC, ICc) == 1; // then the block stages once: no second buffer
        for (int s = 0; s < static_cast<int>(sizeof(shapes) / sizeof(shapes[0])); ++s) {
            const int TB = 1 << shapes[s][0], TH = 1 << shapes[s][1], TW = 1 << shapes[s][2];
            if (preNorm && shapes[s][0] != 0) continue; // the statistics table in LDS is one image's
            const TileLayout L = layout(shapes[s][0], shapes[s][1], shapes[s][2]);
            const size_t lds = oneChunk ? L.ldsBytes / 2 : L.ldsBytes;
            if (L.total > (C8 ? 9 : 5) * 256 || lds > 150 * 1024) continue; // staging registers / LDS
            const double tiles = static_cast<double>(up_div(g.N, TB)) * up_div(g.OH, TH) * up_div(g.OW, TW);
            double cost = tiles * (128.0 * taps + L.total / static_cast<double>(Qs) * 0.5); // MFMA work dominates, staging breaks ties
            if (lds > 80 * 1024) cost *= 1.4;                                 // only one block per CU would fit
            if (best < 0 || cost < bestCost) {
                best = s;
                bestCost = cost;
                bestLds = lds;
            }
        }
    };
    choose();
    // stride-2 halo tiles are ~4x the output tile: with 32-channel (fp32: 16) chunks they take > 80 KB and leave one block per CU (ResNet's
    // downsampling 3x3 convs ran at 28 TF/s fp32 / 90 TF/s fp16).  Half-width chunks double the barriers but keep 2-3 blocks resident.
    // (fp32 also below 80 KB: with a 61 KB double buffer only two 128-pixel blocks fit a CU and the ResNet 56x56 / 7x7 3x3 layers averaged 1.2
    // waves per SIMD; at 48 KB the graph is 1.7 % faster, at 24 KB U-Net loses 4 %.  fp16 layers were 1-2 % slower with the lower bound.)
    size_t narrowAbove = (f16 ? 80 : 48) * 1024;
    if (const char* e = snnhip::option("SNNHIP_CONV_NARROW_KB")) narrowAbove = static_cast<size_t>(atoi(e)) * 1024; // experiments
    bool wideKept = false; // SNNHIP_CONV_WIDE_CHUNKS=1 kept full-width chunks where the default stages half-width ones
    if (C8 == 2 && (best < 0 || bestLds > narrowAbove)) {
        if (!snnhip::option("SNNHIP_CONV_WIDE_CHUNKS")) {
            C8 = 1;
            Qs = 2;
            ICc = 2 * CH;
            choose();
        } else {
            wideKept = true;
        }
    }
    if (best < 0) return SNNHIP_E_UNSUPPORTED;
    MfmaParams p{};
    p.N = g.N; p.H = g.H; p.W = g.W; p.IC = g.IC; p.OC = g.OC; p.kh = g.kh; p.kw = g.kw; p.sh = g.sh; p.sw = g.sw;
    p.padx = g.padx; p.pady = g.pady; p.padMode = g.padMode; p.useBN = g.useBN; p.OH = g.OH; p.OW = g.OW;
    p.preMode = g.preMode; p.preX = g.preX; p.preY = g.preY; p.preShift = g.preMode ? g.preShift : 0;
    p.srcH = g.preMode ? g.srcH : g.H;
    p.srcW = g.preMode ? g.srcW : g.W;
    p.res = nullptr;
    p.statPart = nullptr;
    p.ac2 = make_act_cfg(g.addAct >= 0 ? g.addAct : SNNHIP_ACT_NONE, g.addLeaky);
    p.TBs = shapes[best][0]; p.THs = shapes[best][1]; p.TWs = shapes[best][2];
    const int TB = 1 << p.TBs, TH = 1 << p.THs, TW = 1 << p.TWs;
    const TileLayout L = layout(p.TBs, p.THs, p.TWs);
    p.magicW = static_cast<unsigned>((0x100000000ull + static_cast<unsigned>(L.tileW) - 1) / static_cast<unsigned>(L.tileW));
    p.magicH = static_cast<unsigned>((0x100000000ull + static_cast<unsigned>(L.tileH) - 1) / static_cast<unsigned>(L.tileH));
    p.tileH = L.tileH; p.tileW = L.tileW; p.rowPitch = L.rowPitch; p.imgPitch = L.imgPitch; p.evenCols = L.evenCols;
    p.tilesX = up_div(g.OW, TW);
    p.tilesY = up_div(g.OH, TH);
    p.nChunks = up_div(g.IC, ICc);
    p.total = L.total;
    p.bufFloats = TB * L.imgPitch * Qs * 4;
    const int rNeed = up_div(p.total, 256);
    const int R = (rNeed <= 3 && C8 <= 2) ? 3 : ((rNeed <= 5 && C8 <= 4) ? 5 : 9);

    // Block width and split-K.  Fitted on `SNNHIP_CONV_TUNE=2` logs of the five benchmark graphs (tools/report_tune.py), fp32 and fp16:
    //  * cost model = (rounds of blocks over the CUs) x (output channels per block) x a per-width penalty: narrower blocks re-stage the
    //    activation tile once per block column (worse when the staging goes through a fused Pad / UpSampling address path), the fp16 128-wide
    //    kernel's 2x2 register block (234 VGPRs) leaves two resident blocks per CU where the 64-wide one has three or four;
    //  * fp32, few pixel tiles but a deep reduction (ResNet 14x14 / 7x7 stages, YOLO 13x13, U-Net 16x16): the 128-wide block with the channel
    //    chunks split 4-8 ways over blockIdx.z beats narrow unsplit blocks by 10-25 % (each partial block still streams its A tile once);
    //  (isolated-kernel timings do not transfer one to one: stricter fp16 / shallow-K split rules that won 5-15 % per layer in the tuner's
    //  back-to-back launches lost 5 % on MobileNetV2 and YOLOv3-tiny in the graph, so the split rule below is the conservative one.)
    int BN = 128;
    const int cus = ctx->props.multiProcessorCount > 0 ? ctx->props.multiProcessorCount : 256;
    const double mtiles = static_cast<double>(p.tilesX) * p.tilesY * up_div(g.N, TB);
    const int kdepth = g.IC * taps;
    bool wideSplit = false;
    {
        double bestT = 0;
        const int cands[3] = {128, 64, 32};
        const double penaltyF32[3] = {1.0, 1.08, 1.25}, penaltyF16[3] = {1.15, 1.0, 1.2}, penaltyF16Pre[3] = {1.0, 1.15, 1.4};
        const double* penalty = f16 ? (g.preMode ? penaltyF16Pre : penaltyF16) : penaltyF32;
        for (int c = 0; c < 3; ++c) {
            const double blocks = mtiles * (round_up(g.OC, cands[c]) / cands[c]);
            const double t = std::ceil(blocks / cus) * cands[c] * penalty[c];
            if (c == 0 || t < bestT) {
                bestT = t;
                BN = cands[c];
            }
        }
        if (!f16 && kdepth >= 1024 && g.OC >= 128 && mtiles * up_div(g.OC, 128) < cus) { // split-K fills the chip instead of narrow blocks
            BN = (round_up(g.OC, 128) - g.OC) * 8 > g.OC ? 64 : 128;                     // ... unless 128 pads the channels by > 12.5 %
            wideSplit = true;
        }
    }
    if (const char* e = snnhip::option("SNNHIP_CONV_BN")) // experiments: force the block's output-channel width
        if (atoi(e) == 32 || atoi(e) == 64 || atoi(e) == 128) BN = atoi(e);
    if (ov.bn) BN = ov.bn;
    p.OCp = round_up(g.OC, BN);
    // split-K: deep-K layers with few output tiles (ResNet 14x14 / 7x7 stages at batch 32, MobileNetV2's last pointwise convs) leave most
    // CUs with at most one wave per SIMD; splitting the channel chunks over blockIdx.z gives every SIMD 2+ waves.  Partial sums go to a
    // workspace and a second (element-wise, deterministic) pass applies bias/BN/activation (and the fused residual add, which is cheaper
    // there than in the convolution's epilogue).  SNNHIP_CONV_SPLITK=n forces n (1 = off).
    p.splitK = 1;
    {
        const double blocks = mtiles * (p.OCp / BN);
        int want = 1;
        if (blocks < 1.5 * cus && p.nChunks >= 8) want = static_cast<int>(std::ceil(2.0 * cus / blocks));
        if (want > 8) want = 8;
        const int cap = wideSplit ? p.nChunks / 2 : p.nChunks / 4; // the wide-block rule above relies on the split to fill the chip
        if (want > cap) want = cap;
        if (wideSplit) while (want & (want - 1)) want &= want - 1; // 3x3 layers: 3- / 5-way splits measured 10-25 % behind 2 / 4
        if (const char* e = snnhip::option("SNNHIP_CONV_SPLITK")) want = atoi(e);
        if (ov.splitK) want = ov.splitK;
        if (want < 1 || g.act == SNNHIP_ACT_SILU_QUIRK) want = 1; // the quirk couples 4 adjacent pixels in the epilogue
        if (want > p.nChunks) want = p.nChunks;
        p.chunksPerSplit = up_div(p.nChunks, want);
        p.splitK = up_div(p.nChunks, p.chunksPerSplit);
    }
    // fp16 output tile through LDS (see the kernel's epilogue): needs whole 8-channel vectors and the direct (non split-K) epilogue
    p.ldsEpi = (f16 && p.splitK == 1 && g.OC % 8 == 0 && !snnhip::option("SNNHIP_CONV_DIRECT_STORE")) ? 1 : 0;
    // fp16 with the chunks kept wide by the switch: the K steps of a chunk run half by half (the run-time tap loop has that order), so that the switch
    // changes how the operands are staged and never what is computed
    p.c8Outer = (f16 && wideKept) ? 1 : 0;
    size_t ldsNeed = p.chunksPerSplit == 1 ? L.ldsBytes / 2 : L.ldsBytes; // one chunk per block: no second staging buffer
    p.normShift = g.normShift; p.normMul = g.normMul;
    p.normAc = make_act_cfg(preNorm ? g.normAct : SNNHIP_ACT_NONE, g.normLeaky);
    p.normTabOfs = static_cast<int>(ldsNeed / 4);
    if (preNorm) ldsNeed += static_cast<size_t>(2) * g.IC * sizeof(float); // [shift | mul] behind the staging buffers
    p.coordTabOfs = static_cast<int>(ldsNeed / 4);
    ldsNeed += static_cast<size_t>(p.tileH + p.tileW) * sizeof(int); // the staging's row / column tables
    if (p.ldsEpi) ldsNeed = std::max(ldsNeed, static_cast<size_t>(128) * (BN + 8) * 2);
    const bool simple = act_is_simple(g.act);
    KernelFn fn = nullptr;
    const int staticTaps = p.c8Outer ? 0 : taps; // (the half-by-half order lives in the run-time tap loop)
    if (BN == 128) fn = f16 ? pick_conv2d_mfma_bn128_f16(C8, R, simple, staticTaps) : pick_conv2d_mfma_bn128_f32(C8, R, simple, taps);
    if (BN == 64) fn = f16 ? pick_conv2d_mfma_bn64_f16(C8, R, simple, staticTaps) : pick_conv2d_mfma_bn64_f32(C8, R, simple, taps);
    if (BN == 32) fn = f16 ? pick_conv2d_mfma_bn32_f16(C8, R, simple, staticTaps) : pick_conv2d_mfma_bn32_f32(C8, R, simple, taps);
    if (!fn) return SNNHIP_E_UNSUPPORTED;

    auto* plan = new MfmaConvPlan();
    plan->ctx = ctx;
    plan->g = g;
    plan->w_oihw.assign(w_oihw, w_oihw + static_cast<size_t>(g.OC) * g.IC * taps);
    plan->epi4 = epi4;
    plan->p = p;
    plan->ac = make_act_cfg(g.act, g.leaky);
    plan->kernel = fn;
    plan->ldsBytes = ldsNeed;
    plan->fusedAdd = g.addAct >= 0;
    if (plan->fusedAdd) plan->numInputs = 2;
    plan->grid = dim3(p.tilesX * p.tilesY * up_div(g.N, TB), p.OCp / BN, p.splitK);
    if (p.splitK > 1) {
        void* ws = nullptr;
        const size_t wsBytes = static_cast<size_t>(p.splitK) * g.N * g.OH * g.OW * g.OC * sizeof(float);
        if (snnhip::dev_malloc(&ws, wsBytes) != hipSuccess) {
            set_error("conv2d_mfma: split-K workspace of %zu bytes", wsBytes);
            delete plan;
            return SNNHIP_E_HIP;
        }
        plan->deviceAllocs.push_back(ws);
        plan->d_ws = static_cast<float*>(ws);
    }
    if (ldsNeed > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(ldsNeed));
        if (e != hipSuccess) {
            set_error("hipFuncSetAttribute(%zu) failed: %s", ldsNeed, hipGetErrorString(e));
            delete plan;
            return SNNHIP_E_HIP;
        }
    }

    // weights: Wp[chunk][tap][c8][h][OCp][j] (c8Outer: Wp[chunk][c8][tap]...), ic = chunk*ICc + (c8*2 + h)*CH + j, j < CH (+ 10 zero steps: the prefetch ring reads up to 9
    // steps ahead); 16 bytes per (h, oc): 4 floats or 8 halfs (fp32 -> fp16 rounds to nearest; weights that went through the reference's
    // truncating convertToMediumPrecision are representable and convert exactly)
    const size_t steps = C8 ? static_cast<size_t>(p.nChunks) * taps * C8 : static_cast<size_t>((taps + 1) / 2);
    std::vector<float> wpk((steps + 10) * 2 * p.OCp * 4, 0.0f); // 16 bytes per (step, h, oc) in both precisions; 10 >= the deepest ring
    _Float16* wph = reinterpret_cast<_Float16*>(wpk.data());
    if (C8 == 0) { // tap-pair mode: Wp[step j][h][OCp][ic], tap = 2j + h
        for (int t = 0; t < taps; ++t)
            for (int j = 0; j < g.IC; ++j) {
                const size_t base = (static_cast<size_t>(t / 2) * 2 + (t & 1)) * p.OCp;
                for (int o = 0; o < g.OC; ++o) {
                    const float wv = w_oihw[(static_cast<size_t>(o) * g.IC + j) * taps + t];
                    if (f16) wph[(base + o) * 8 + j] = static_cast<_Float16>(wv);
                    else wpk[(base + o) * 4 + j] = wv;
                }
            }
    }
    for (int chunk = 0; chunk < p.nChunks; ++chunk)
        for (int t = 0; t < taps; ++t)
            for (int c8 = 0; c8 < C8; ++c8)
                for (int hh = 0; hh < 2; ++hh)
                    for (int j = 0; j < CH; ++j) {
                        const int ic = chunk * ICc + (c8 * 2 + hh) * CH + j;
                        if (ic >= g.IC) continue;
                        const size_t step = p.c8Outer ? (static_cast<size_t>(chunk) * C8 + c8) * taps + t : (static_cast<size_t>(chunk) * taps + t) * C8 + c8;
                        const size_t base = (step * 2 + hh) * p.OCp;
                        for (int o = 0; o < g.OC; ++o) {
                            const float wv = w_oihw[(static_cast<size_t>(o) * g.IC + ic) * taps + t];
                            if (f16) wph[(base + o) * 8 + j] = static_cast<_Float16>(wv);
                            else wpk[(base + o) * 4 + j] = wv;
                        }
                    }
    std::vector<float> epiP(static_cast<size_t>(p.OCp) * 4, 0.0f);
    std::memcpy(epiP.data(), epi4.data(), sizeof(float) * 4 * static_cast<size_t>(g.OC));
    int rc = plan->upload(wpk.data(), wpk.size(), &plan->d_w);
    if (rc == SNNHIP_OK) rc = plan->upload(epiP.data(), epiP.size(), &plan->d_epi);
    if (rc != SNNHIP_OK) {
        delete plan;
        return rc;
    }
    plan->inDims[0] = g.N; plan->inDims[1] = p.srcH; plan->inDims[2] = p.srcW; plan->inDims[3] = g.IC;
    plan->outDims[0] = g.N; plan->outDims[1] = g.OH; plan->outDims[2] = g.OW; plan->outDims[3] = g.OC;
    plan->flops = 2.0 * taps * g.IC * g.OC * static_cast<double>(g.OH) * g.OW * g.N;
    plan->bytes = 4.0 * (static_cast<double>(g.N) * g.H * g.W * g.IC + static_cast<double>(g.N) * g.OH * g.OW * g.OC +
                         static_cast<double>(g.OC) * g.IC * taps);
    char buf[256];
    char chunkDesc[24];
    if (C8) snprintf(chunkDesc, sizeof(chunkDesc), "chunk=%d", ICc);
    else snprintf(chunkDesc, sizeof(chunkDesc), "tap-pairs");
    snprintf(buf, sizeof(buf), "conv2d_mfma_%s k=%dx%d s=%d ic=%d oc=%d tile=%dx%dx%dpx x %doc %s lds=%zuB splitK=%d",
             f16 ? "f16_32x32x16" : "f32_32x32x2", g.kh, g.kw, g.sh, g.IC, g.OC, TB, TH, TW, BN, chunkDesc, ldsNeed, p.splitK);
    plan->dtype = g.dtype;
    const double esz = f16 ? 2.0 : 4.0;
    plan->bytes = esz * (static_cast<double>(g.N) * p.srcH * p.srcW * g.IC + static_cast<double>(g.N) * g.OH * g.OW * g.OC + static_cast<double>(g.OC) * g.IC * taps);
    plan->desc = buf;
    if (g.preMode) plan->desc += " +pad(" + std::string(g.preMode == SNNHIP_PAD_REFLECT ? "reflect" : g.preMode == SNNHIP_PAD_REPLICATE ? "replicate" : "constant") + ")";
    if (g.preMode && g.preShift) plan->desc += " +upsample(x2)";
    if (plan->fusedAdd) {
        plan->desc += " +add";
        plan->bytes += esz * static_cast<double>(g.N) * g.OH * g.OW * g.OC; // the residual is read once
    }
    if (preNorm) plan->desc = "instancenorm(act=" + std::to_string(g.normAct) + ", in the staging) -> " + plan->desc;
    *out = plan;
    return SNNHIP_OK;
}

// Public entry: the heuristic configuration, or -- SNNHIP_CONV_TUNE=1 -- the fastest of a few (block width, split-K) candidates timed on the
// device at plan creation (5 launches each on scratch tensors; the winner per geometry is cached for the life of the process).  The
// heuristics were fitted on a handful of shapes; measured on the ResNet-18 body (fp16, batch 32) the best candidate is 10-25 % faster on
// the 28x28 / 14x14 / 7x7 stages, where block count, residency and the split-K reduce pass trade against each other.
int make_conv2d_mfma_plan(snnhip_ctx* ctx, const ConvGeom& g, const float* w_oihw, const std::vector<float>& epi4, snnhip_plan** out) {
    // fp32 3x3 stride-1 layers with GEMM-sized channel counts: Winograd F(2x2,3x3) on the matrix pipe (conv2d_wino.hip), 2.25x fewer MFMA
    // flops than the implicit GEMM below.  SNNHIP_CONV=wino forces it for every eligible shape, SNNHIP_CONV=mfma / SNNHIP_CONV_WINO=0 keep
    // the direct kernel (tests run both on the same inputs).
    {
        const char* force = snnhip::option("SNNHIP_CONV");
        const char* w = snnhip::option("SNNHIP_CONV_WINO");
        const bool forced = force && strcmp(force, "wino") == 0;
        const bool allowed = !force && !(w && atoi(w) == 0) && !snnhip::option("SNNHIP_CONV_BN") && !snnhip::option("SNNHIP_CONV_C8") && g.IC >= 32 && g.OC >= 32 && !g.normShift;
        if (forced || allowed) {
            const int rc = make_conv2d_wino_plan(ctx, g, w_oihw, epi4, out);
            if (rc != SNNHIP_E_UNSUPPORTED || forced) return rc;
        }
    }
    // fp32 3x3 stride-2 layers with GEMM-sized channel counts: the K axis split over the waves of a block, operands straight from the L2, partial
    // tiles summed through LDS (conv2d_ksplit.hip) -- one launch where the kernel below needs split-K over blockIdx.z + a reduce pass.
    // SNNHIP_CONV=ksplit forces it for every eligible shape (any kernel size / stride), SNNHIP_CONV=mfma / SNNHIP_CONV_KSPLIT=0 keep the split-K kernel.
    {
        const char* force = snnhip::option("SNNHIP_CONV");
        const char* w = snnhip::option("SNNHIP_CONV_KSPLIT");
        const bool forced = force && strcmp(force, "ksplit") == 0;
        const bool allowed = !force && !(w && atoi(w) == 0) && !snnhip::option("SNNHIP_CONV_BN") && !snnhip::option("SNNHIP_CONV_SPLITK") && !snnhip::option("SNNHIP_CONV_C8") &&
                             !snnhip::option("SNNHIP_CONV_1X1"); // (a pinned pointwise kernel stays pinned)
        if (forced || allowed) {
            const int rc = make_conv2d_ksplit_plan(ctx, g, w_oihw, epi4, out);
            if (rc != SNNHIP_E_UNSUPPORTED || forced) return rc;
        }
    }
    // the RGB stems (IC <= 4): conv2d_stem_f16.hip (fp16 9x9 stride 1) and conv2d_stem_f32.hip (fp32 3x3 stride 1 / 2, 7x7 stride 2)
    {
        int rc = make_conv2d_stem_plan(ctx, g, w_oihw, epi4, out);
        if (rc == SNNHIP_E_UNSUPPORTED) rc = make_conv2d_stem32_plan(ctx, g, w_oihw, epi4, out);
        if (rc != SNNHIP_E_UNSUPPORTED) return rc;
    }
    // fp16 nearest x2 UpSampling -> reflect Pad(1) -> 3x3 (rule D's fused geometry): 4 phases x 2x2 taps on the low-resolution tensor (conv2d_upconv.hip;
    // SNNHIP_CONV=upconv forces it for every eligible shape, SNNHIP_CONV_UPCONV=0 keeps the 9-tap kernels)
    if (g.preShift == 1) {
        const char* force = snnhip::option("SNNHIP_CONV");
        const char* w = snnhip::option("SNNHIP_CONV_UPCONV");
        const bool forced = force && strcmp(force, "upconv") == 0;
        const bool allowed = !force && !(w && atoi(w) == 0) && !snnhip::option("SNNHIP_CONV_BN") && !snnhip::option("SNNHIP_CONV_SPLITK") && !snnhip::option("SNNHIP_CONV_C8");
        if (forced || allowed) {
            const int rc = make_conv2d_upconv_plan(ctx, g, w_oihw, epi4, out);
            if (rc != SNNHIP_E_UNSUPPORTED) return rc;
        }
    }
    // fp16 3x3 stride-1 layers on large maps: the 4 x 2 register-block kernel of conv2d_wide_f16.hip (SNNHIP_CONV=wide forces it for every
    // eligible shape, SNNHIP_CONV=mfma / SNNHIP_CONV_WIDE=0 keep the 128-pixel kernel)
    {
        const char* force = snnhip::option("SNNHIP_CONV");
        const char* w = snnhip::option("SNNHIP_CONV_WIDE");
        const bool forced = force && strcmp(force, "wide") == 0;
        const bool allowed = !force && !(w && atoi(w) == 0) && !snnhip::option("SNNHIP_CONV_BN") && !snnhip::option("SNNHIP_CONV_SPLITK") && !snnhip::option("SNNHIP_CONV_C8");
        if (forced || allowed) {
            const int rc = make_conv2d_wide_plan(ctx, g, w_oihw, epi4, out);
            if (rc != SNNHIP_E_UNSUPPORTED || forced) return rc;
        }
    }
    // fp16 3x3 stride-2 layers with 32 / 64 input channels on large maps: the row-marching strips of conv2d_s2march.hip (SNNHIP_CONV=s2march forces it
    // for every eligible shape, SNNHIP_CONV=mfma / SNNHIP_CONV_S2MARCH=0 keep the 128-pixel kernel)
    {
        const char* force = snnhip::option("SNNHIP_CONV");
        const char* w = snnhip::option("SNNHIP_CONV_S2MARCH");
        const bool forced = force && strcmp(force, "s2march") == 0;
        const bool allowed = !force && !(w && atoi(w) == 0) && !snnhip::option("SNNHIP_CONV_BN") && !snnhip::option("SNNHIP_CONV_SPLITK") && !snnhip::option("SNNHIP_CONV_C8");
        if (forced || allowed) {
            const int rc = make_conv2d_s2march_plan(ctx, g, w_oihw, epi4, out);
            if (rc != SNNHIP_E_UNSUPPORTED || forced) return rc;
        }
    }
    // pointwise layers (fp32, and fp16 with OC % 8 == 0) stream through conv1x1_stream.hip (no halo tile to stage); forcing a kernel or a
    // configuration skips it
    if (!snnhip::option("SNNHIP_CONV") && !snnhip::option("SNNHIP_CONV_BN") && !snnhip::option("SNNHIP_CONV_SPLITK") && !snnhip::option("SNNHIP_CONV_C8")) {
        const int rc = make_conv1x1_stream_plan(ctx, g, w_oihw, epi4, out);
        if (rc != SNNHIP_E_UNSUPPORTED) return rc;
    }
    const char* tune = snnhip::option("SNNHIP_CONV_TUNE");
    if (!tune || atoi(tune) == 0 || snnhip::option("SNNHIP_CONV_BN") || snnhip::option("SNNHIP_CONV_SPLITK")) return make_conv2d_mfma_plan_ex(ctx, g, w_oihw, epi4, MfmaOverride(), out);
    // winners are cached per (device, full geometry incl. the output extent, epilogue shape); the cache is shared by every context of the
    // process, so it is guarded (plan creation may run on several host threads, one per device)
    char key[320];
    snprintf(key, sizeof(key), "d%d.%d.%d.%d.%d.%d.%d.%d.%d.%d.%d.%d.%d.%d.%d.%d.%d.%d.%d.%d.%d.%d", ctx->device, g.N, g.H, g.W, g.IC, g.OC, g.kh, g.kw, g.sh, g.sw,
             g.padx, g.pady, g.dtype, g.preMode, g.preShift, g.srcH, g.srcW, g.addAct >= 0, g.OH, g.OW, g.act, g.useBN);
    static std::map<std::string, MfmaOverride> cache;
    static std::mutex cacheMutex;
    {
        std::lock_guard<std::mutex> lock(cacheMutex);
        auto it = cache.find(key);
        if (it != cache.end()) {
            const MfmaOverride hit = it->second;
            return make_conv2d_mfma_plan_ex(ctx, g, w_oihw, epi4, hit, out);
        }
    }

    const size_t esz = g.dtype == SNNHIP_F16 ? 2 : 4;
    const size_t inBytes = static_cast<size_t>(g.N) * (g.preMode ? g.srcH : g.H) * (g.preMode ? g.srcW : g.W) * g.IC * esz;
    const size_t outBytes = static_cast<size_t>(g.N) * g.OH * g.OW * g.OC * esz;
    void *dx = nullptr, *dy = nullptr, *dr = nullptr;
    if (snnhip::dev_malloc(&dx, inBytes) != hipSuccess || snnhip::dev_malloc(&dy, outBytes) != hipSuccess || (g.addAct >= 0 && snnhip::dev_malloc(&dr, outBytes) != hipSuccess)) {
        if (dx) (void) snnhip::dev_free(dx);
        if (dy) (void) snnhip::dev_free(dy);
        return make_conv2d_mfma_plan_ex(ctx, g, w_oihw, epi4, MfmaOverride(), out);
    }
    bool hipOk = hipMemsetAsync(dx, 0, inBytes, ctx->stream) == hipSuccess;
    if (dr) hipOk = hipOk && hipMemsetAsync(dr, 0, outBytes, ctx->stream) == hipSuccess;
    snnhip_tensor tx, ty, tr;
    tx.ctx = ty.ctx = tr.ctx = ctx;
    tx.n = g.N; tx.h = g.preMode ? g.srcH : g.H; tx.w = g.preMode ? g.srcW : g.W; tx.c = g.IC; tx.dtype = g.dtype; tx.data = static_cast<float*>(dx);
    ty.n = g.N; ty.h = g.OH; ty.w = g.OW; ty.c = g.OC; ty.dtype = g.dtype; ty.data = static_cast<float*>(dy);
    tr = ty;
    tr.data = static_cast<float*>(dr);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipOk = hipOk && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
    if (!hipOk) { // the tuner is an optimisation: any HIP failure here falls back to the heuristic configuration
        if (e0) (void) hipEventDestroy(e0);
        if (e1) (void) hipEventDestroy(e1);
        (void) snnhip::dev_free(dx);
        (void) snnhip::dev_free(dy);
        if (dr) (void) snnhip::dev_free(dr);
        return make_conv2d_mfma_plan_ex(ctx, g, w_oihw, epi4, MfmaOverride(), out);
    }
    MfmaOverride best;
    float bestMs = -1.0f;
    const int bns[4] = {0, 32, 64, 128};
    const int splits[4] = {0, 1, 2, 4};
    std::string seen;
    for (int bi = 0; bi < 4; ++bi)
        for (int si = 0; si < 4; ++si) {
            if (bns[bi] > round_up(g.OC, 32) && bns[bi] != 32) continue; // wider than the layer: pure padding
            MfmaOverride ov;
            ov.bn = bns[bi];
            ov.splitK = splits[si];
            snnhip_plan* cand = nullptr;
            if (make_conv2d_mfma_plan_ex(ctx, g, w_oihw, epi4, ov, &cand) != SNNHIP_OK) continue;
            if (seen.find("|" + cand->desc + "|") != std::string::npos) { // same configuration as an earlier candidate
                delete cand;
                continue;
            }
            seen += "|" + cand->desc + "|";
            const snnhip_tensor* ins[2] = {&tx, &tr};
            const int nIn = g.addAct >= 0 ? 2 : 1;
            bool ok = cand->run(ins, nIn, &ty) == SNNHIP_OK; // warm-up
            float ms = 0.0f;
            for (int round = 0; round < 2 && ok; ++round) { // the better of two 5-launch timings: clocks wander on a busy box
                (void) hipEventRecord(e0, ctx->stream);
                for (int r = 0; r < 5 && ok; ++r) ok = cand->run(ins, nIn, &ty) == SNNHIP_OK;
                (void) hipEventRecord(e1, ctx->stream);
                float t = 0.0f;
                if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&t, e0, e1) != hipSuccess) ok = false;
                if (round == 0 || t < ms) ms = t;
            }
            if (atoi(tune) >= 2) // SNNHIP_CONV_TUNE=2: log every candidate (the data the heuristics above are fitted on)
                fprintf(stderr, "[snnhip tune] N=%d %dx%d ic=%d oc=%d k=%d s=%d %s | bn=%d splitK=%d -> %s : %.1f us%s\n", g.N, g.H, g.W, g.IC, g.OC, g.kh, g.sh,
                        g.dtype == SNNHIP_F16 ? "f16" : "f32", ov.bn, ov.splitK, cand->desc.c_str(), ok ? ms * 200.0f : -1.0f, (bi == 0 && si == 0) ? " (heuristic)" : "");
            delete cand;
            if (ok && (bestMs < 0.0f || ms < bestMs)) {
                bestMs = ms;
                best = ov;
            }
        }
    (void) hipEventDestroy(e0);
    (void) hipEventDestroy(e1);
    (void) hipStreamSynchronize(ctx->stream);
    (void) snnhip::dev_free(dx);
    (void) snnhip::dev_free(dy);
    if (dr) (void) snnhip::dev_free(dr);
    {
        std::lock_guard<std::mutex> lock(cacheMutex);
        cache[key] = best;
    }
    return make_conv2d_mfma_plan_ex(ctx, g, w_oihw, epi4, best, out);
}

} // namespace snnhip
