// conv2d_wide_f16.hip -- fp16 3x3 stride-1 convolution for large feature maps (the bodies of the style-transfer / U-Net graphs): the implicit
// GEMM of conv2d_mfma.hip with a 4 x NT register block of v_mfma_f32_32x32x16_f16 tiles per wave (128 pixels x 64 / 32 output channels)
// instead of 2 x 2.
//
// Why a second kernel (measured on Candy 720p fp16, tools/gpu_candy_abl.sh): the 128-pixel blocks of conv2d_mfma_kernel reach 23 % of the
// fp16 matrix peak on the 128 -> 128 layers and 57 % with every memory operation ablated.  One 32x32x16 MFMA consumes 2 KB of operands in 32
// cycles; a CU's four SIMDs would need 256 B/clk with no reuse, LDS delivers 128 B/clk and the vector L1 64 B/clk.  With a 2 x 2 register
// block the activation operands cost 64 B/clk of LDS reads and the weights (streamed per lane from L2) 64 B/clk of L1 -- the L1 is saturated
// at HALF the matrix rate before the halo-tile staging asks for anything.  A 4 x 2 block halves the weight stream (32 B/clk) at the same LDS
// rate, a 256-pixel block tile halves the weight traffic per output once more, and the unrolled K loop spends 8 MFMAs (256 cycles) per LDS /
// L1 round trip instead of 4.
//
//   * block = 256 threads = WM x WN waves, pixel tile TH x 32 (TH = 8 or 16) of ONE image, BN = 32 NT WN output channels:
//       WM=2 WN=2 NT=2: 256 px x 128 oc     WM=4 WN=1 NT=2: 512 px x 64 oc     WM=4 WN=1 NT=1: 512 px x 32 oc
//   * halo tile staged through registers into LDS in channel chunks of 16 C8 (double-buffered, one barrier per chunk), XOR-swizzled 16-byte
//     slots as in conv2d_mfma_kernel (lds_off); the fused Pad / UpSampling address path (ConvGeom::preMode / preShift) resolves here;
//   * graph rule I (the InstanceNorm in front folded into this layer): the DMA carries the raw values, every thread then normalises the slots
//     its own lanes copied, in LDS, before the barrier that publishes the chunk (norm_fixup below);
//   * weights packed exactly as for conv2d_mfma_kernel ([chunk][tap][c8][h][OCp] x 8 halfs), streamed per lane with a 3-step ring;
//   * the weights are the MFMA's A operand, the pixels its B operand: a lane ends up with runs of 4 consecutive output channels of its own
//     pixel and the epilogue (bias / BN / activation / fused residual Add) stores them directly, 8 bytes per lane, without an LDS transpose.
#include "conv2d_mfma_kernel.h"
#include "norm_fold.h"

#include <cstring>

#ifndef SNNHIP_WIDE_ABL
#define SNNHIP_WIDE_ABL 0 // ablation builds only (tools/ablate_wide.sh): 1 no weight refills, 2 no LDS operand reads, 4 no activation DMA, 8 no output stores
#endif

#ifdef SNNHIP_WIDE_TRACE // experiment builds (tools/exp_one.sh): one block prints the s_memtime stamps of its phases
#define WIDE_MARK(i) do { if (wtrace) wstamp[i] = __builtin_readcyclecounter(); } while (0)
#else
#define WIDE_MARK(i) do { } while (0)
#endif

namespace snnhip {

namespace {

using mfma_detail::f32x16;

struct WideParams {
    int N, H, W, IC, OC, padx, pady, padMode, useBN, OH, OW;
    int THs;             // log2 of the tile height; the tile is (1 << THs) x 32 pixels
    int tileH, tileW;    // staged halo tile
    int tilesX, tilesY;
    int nChunks, OCp, total, bufFloats;
    int epiOfs;          // float offset in LDS of the block's epilogue-table rows
    int zeroOfs;         // float4 offset (from the packed weights) of a block of zeros: source of the padding pixels' DMA
    int preMode, preX, preY, srcH, srcW, preShift;
    unsigned magicW;
    const void* res; // fused residual Add (chain rule E)
    ActCfg ac2;
    float* statPart; // chain rule F: per (image, tile, channel) {mean, M2} of the stored values, [n][ty][tx][2][OC]; null = off
    NormFoldArgs fold; // ... and the last block of an image folds them into the norm's shift / mul (norm_fold.h); fold.counter == null = off
    // graph rule I: the InstanceNorm in front, normAc(x * mul[n][c] + shift[n][c]), applied to the staged values IN LDS (below); null = none
    const float* normShift;
    const float* normMul;
    ActCfg normAc;
    // K-loop token (round 4): the two blocks a CU holds lock-step -- both in their K loops (the matrix pipe shared), then both in prologue / epilogue
    // / stores (the pipe idle): 0.45 busy over the launch.  kTok[physical CU] is a mutual exclusion around the K loop: a block takes it before its
    // first chunk and returns it after its last, so a CU's blocks ALTERNATE (one multiplies at the full pipe rate while the other stages / stores).
    // Purely a performance device: a token shared by blocks of different CUs (an aliased id) only serialises them.  null = off.
    unsigned* kTok;
};

// physical CU of the calling wave, hashed to [0, 2048): XCC id (8) x the SE / SH / CU fields of HW_ID (bits 8..15)
__device__ __forceinline__ unsigned physical_cu_slot() {
    const unsigned hw = __builtin_amdgcn_s_getreg((4) | (8 << 6) | (7 << 11));   // HW_REG_HW_ID, 8 bits from bit 8: cu_id, sh_id, se_id (bit 16 up: the workgroup slot)
    const unsigned xcc = __builtin_amdgcn_s_getreg((20) | (0 << 6) | (3 << 11)); // HW_REG_XCC_ID, 4 bits
    return ((xcc & 7u) << 8) | (hw & 255u);
}
constexpr int kTokSlots = 2048;

// CAT (chain rule K: Concatenate -> Conv2D, conv2d_wide_cat_kernel below): the K chunks come from TWO tensors of the convolution's own extent.  A chunk is
// 16 C8 channels and C0 a multiple of that, so a chunk lies wholly in one source; the staged pixel (rowPix + sx) is the same in both, only the base pointer,
// the pixel pitch and the channel origin change -- block-uniform values chosen per chunk in stage_dma, the lane's address one multiply-add on its pixel index.
// The DMA count per chunk (R per thread) is that of the single-source kernel: the counted vmcnt behind the K steps holds unchanged.
struct WideCatParams {
    const _Float16* x1; // input 1: [N][H][W][IC - C0] (input 0 is the kernel's x: [N][H][W][C0])
    int C0;             // channels taken from input 0 = its pixel pitch
};

// POOL (chain rule L: Conv2D -> MaxPooling2D 2x2 stride 2, conv2d_wide_pool_kernel below): the K loop, the LDS-DMA staging and the counted vmcnt are the plain
// kernel's; only the epilogue behind the loop's last barrier differs (conv2d_wide_body.h: the vertical maximum in registers, the horizontal one at the read-out).
struct WidePoolParams {
    int poolOH, poolOW; // the pooling plan's own output extent: ceil or floor of OH / 2, OW / 2
};

template <int WM, int WN, int NT, int C8, int R, bool SIMPLE, bool RES>
__global__ __launch_bounds__(256, 2) void conv2d_wide_kernel(WideParams p, ActCfg ac, const _Float16* __restrict__ x, const float4* __restrict__ wp,
                                                          const float4* __restrict__ epi, _Float16* __restrict__ y) {
    constexpr bool CAT = false, POOL = false;
    const WideCatParams cp = {}; // (unused: every use sits behind CAT)
    const WidePoolParams pq = {}; // (... behind POOL)
#include "conv2d_wide_body.h"
}
// the two-source instances (chain rule K); x = input 0, cp.x1 = input 1
template <int WM, int WN, int NT, int C8, int R, bool SIMPLE>
__global__ __launch_bounds__(256, 2) void conv2d_wide_cat_kernel(WideParams p, WideCatParams cp, ActCfg ac, const _Float16* __restrict__ x, const float4* __restrict__ wp,
                                                              const float4* __restrict__ epi, _Float16* __restrict__ y) {
    constexpr bool RES = false, CAT = true, POOL = false;
    const WidePoolParams pq = {};
#include "conv2d_wide_body.h"
}
// the pooling instances (chain rule L: the simple activations only); y = [N][pq.poolOH][pq.poolOW][OC]
template <int WM, int WN, int NT, int C8, int R>
__global__ __launch_bounds__(256, 2) void conv2d_wide_pool_kernel(WideParams p, WidePoolParams pq, ActCfg ac, const _Float16* __restrict__ x, const float4* __restrict__ wp,
                                                               const float4* __restrict__ epi, _Float16* __restrict__ y) {
    constexpr bool SIMPLE = true, RES = false, CAT = false, POOL = true;
    const WideCatParams cp = {};
#include "conv2d_wide_body.h"
}

typedef void (*WideFn)(WideParams, ActCfg, const _Float16*, const float4*, const float4*, _Float16*);
typedef void (*WideCatFn)(WideParams, WideCatParams, ActCfg, const _Float16*, const float4*, const float4*, _Float16*);
typedef void (*WidePoolFn)(WideParams, WidePoolParams, ActCfg, const _Float16*, const float4*, const float4*, _Float16*);

struct WideConvPlan : ConvPlanBase {
    WideParams p;
    ActCfg ac;
    float* d_w = nullptr;
    float* d_epi = nullptr;
    size_t ldsBytes = 0;
    dim3 grid;
    WideFn kernel = nullptr;
    WideCatFn catKernel = nullptr; // chain rule K (g.C0 > 0): the two-source instance, cp its parameter block
    WideCatParams cp = {};
    bool fusedAdd = false;
    WidePoolFn poolKernel = nullptr; // chain rule L (g.poolOH > 0): the output is the pooled tensor
    WidePoolParams pq = {};

    // chain rule F: {mean, M2} of every output tile and channel next to the output (the epilogue's LDS round trip carries them: conv2d_wide_kernel)
    bool enableTileStats() override {
        if (statPart) return true;
        if (poolKernel) return false; // (rule L: the pooling epilogue leaves before the statistics)
        if (fusedAdd) return false; // (rule E: the kernel instantiation with the residual carries no statistics code)
        void* buf = nullptr;
        const size_t bytes = static_cast<size_t>(p.N) * p.tilesY * p.tilesX * 2 * p.OC * sizeof(float);
        if (snnhip::dev_malloc(&buf, bytes) != hipSuccess) return false;
        deviceAllocs.push_back(buf);
        statPart = p.statPart = static_cast<float*>(buf);
        statTilesX = p.tilesX; statTilesY = p.tilesY; statTH = 1 << p.THs; statTW = 32;
        desc += " +tile-stats";
        return true;
    }
    bool enableNormFold(const NormFoldTarget& t) override {
        if (!statPart || p.fold.counter) return false;
        void* buf = nullptr;
        const size_t bytes = static_cast<size_t>(p.N) * grid.y * sizeof(unsigned);
        if (snnhip::dev_malloc(&buf, bytes) != hipSuccess) return false;
        deviceAllocs.push_back(buf);
        if (hipMemset(buf, 0, bytes) != hipSuccess) return false;
        p.fold.counter = static_cast<unsigned*>(buf);
        p.fold.gamma = t.gamma; p.fold.beta = t.beta; p.fold.shift = t.shift; p.fold.mul = t.mul; p.fold.eps = t.eps;
        desc += "+fold";
        return true;
    }
    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        if (catKernel) { // chain rule K: two inputs in the concat's order, both at the convolution's extent
            SNNHIP_REQUIRE(nIn == 2, "conv2d+concat: expects 2 inputs, got %d", nIn);
            for (int s = 0; s < 2; ++s) {
                const int c = s ? p.IC - cp.C0 : cp.C0;
                SNNHIP_REQUIRE(in[s]->n == p.N && in[s]->h == p.H && in[s]->w == p.W && in[s]->c == c && in[s]->dtype == SNNHIP_F16,
                               "conv2d+concat: input %d dims %dx%dx%dx%d (dtype %d) != plan %dx%dx%dx%d fp16", s, in[s]->n, in[s]->h, in[s]->w, in[s]->c, in[s]->dtype, p.N, p.H, p.W, c);
            }
            SNNHIP_REQUIRE(out->n == p.N && out->h == p.OH && out->w == p.OW && out->c == p.OC && out->dtype == SNNHIP_F16,
                           "conv2d: output dims %dx%dx%dx%d != plan %dx%dx%dx%d", out->n, out->h, out->w, out->c, p.N, p.OH, p.OW, p.OC);
            WideCatParams c2 = cp;
            c2.x1 = reinterpret_cast<const _Float16*>(in[1]->data);
            SNNHIP_LAUNCH(catKernel, grid, dim3(256), ldsBytes, ctx->stream, p, c2, ac, reinterpret_cast<const _Float16*>(in[0]->data), reinterpret_cast<const float4*>(d_w),
                               reinterpret_cast<const float4*>(d_epi), reinterpret_cast<_Float16*>(out->data));
            SNNHIP_CHECK_HIP(hipGetLastError());
            return SNNHIP_OK;
        }
        if (poolKernel) { // chain rule L: one input, the pooled output
            SNNHIP_REQUIRE(nIn == 1, "conv2d+maxpool: expects 1 input, got %d", nIn);
            SNNHIP_REQUIRE(in[0]->n == p.N && in[0]->h == p.H && in[0]->w == p.W && in[0]->c == p.IC && in[0]->dtype == SNNHIP_F16,
                           "conv2d+maxpool: input dims %dx%dx%dx%d (dtype %d) != plan %dx%dx%dx%d fp16", in[0]->n, in[0]->h, in[0]->w, in[0]->c, in[0]->dtype, p.N, p.H, p.W, p.IC);
            SNNHIP_REQUIRE(out->n == p.N && out->h == pq.poolOH && out->w == pq.poolOW && out->c == p.OC && out->dtype == SNNHIP_F16,
                           "conv2d+maxpool: output dims %dx%dx%dx%d (dtype %d) != plan %dx%dx%dx%d fp16", out->n, out->h, out->w, out->c, out->dtype, p.N, pq.poolOH, pq.poolOW, p.OC);
            SNNHIP_LAUNCH(poolKernel, grid, dim3(256), ldsBytes, ctx->stream, p, pq, ac, reinterpret_cast<const _Float16*>(in[0]->data), reinterpret_cast<const float4*>(d_w),
                               reinterpret_cast<const float4*>(d_epi), reinterpret_cast<_Float16*>(out->data));
            SNNHIP_CHECK_HIP(hipGetLastError());
            return SNNHIP_OK;
        }
        SNNHIP_REQUIRE(nIn == (fusedAdd ? 2 : 1), "conv2d: expects %d input(s), got %d", fusedAdd ? 2 : 1, nIn);
        const snnhip_tensor* x = in[0];
        WideParams q = p;
        q.res = nullptr;
        if (fusedAdd) {
            const snnhip_tensor* r = in[1];
            SNNHIP_REQUIRE(r->n == p.N && r->h == p.OH && r->w == p.OW && r->c == p.OC && r->dtype == dtype,
                           "conv2d+add: residual %dx%dx%dx%d (dtype %d) does not match the output %dx%dx%dx%d", r->n, r->h, r->w, r->c, r->dtype, p.N, p.OH,
                           p.OW, p.OC);
            q.res = r->data;
        }
        SNNHIP_REQUIRE(x->n == p.N && x->h == p.srcH && x->w == p.srcW && x->c == p.IC && x->dtype == SNNHIP_F16,
                       "conv2d: input dims %dx%dx%dx%d (dtype %d) != plan %dx%dx%dx%d fp16", x->n, x->h, x->w, x->c, x->dtype, p.N, p.srcH, p.srcW, p.IC);
        SNNHIP_REQUIRE(out->n == p.N && out->h == p.OH && out->w == p.OW && out->c == p.OC && out->dtype == SNNHIP_F16,
                       "conv2d: output dims %dx%dx%dx%d != plan %dx%dx%dx%d", out->n, out->h, out->w, out->c, p.N, p.OH, p.OW, p.OC);
        SNNHIP_LAUNCH(kernel, grid, dim3(256), ldsBytes, ctx->stream, q, ac, reinterpret_cast<const _Float16*>(x->data), reinterpret_cast<const float4*>(d_w),
                           reinterpret_cast<const float4*>(d_epi), reinterpret_cast<_Float16*>(out->data));
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }
};

template <int WM, int WN, int NT, int C8, int R>
WideFn pick_wide(bool simple, bool res) {
    if (res) return simple ? conv2d_wide_kernel<WM, WN, NT, C8, R, true, true> : conv2d_wide_kernel<WM, WN, NT, C8, R, false, true>;
    return simple ? conv2d_wide_kernel<WM, WN, NT, C8, R, true, false> : conv2d_wide_kernel<WM, WN, NT, C8, R, false, false>;
}
template <int WM, int WN, int NT, int C8, int R>
WideCatFn pick_wide_cat(bool simple) {
    return simple ? conv2d_wide_cat_kernel<WM, WN, NT, C8, R, true> : conv2d_wide_cat_kernel<WM, WN, NT, C8, R, false>;
}

} // namespace

// where this kernel is tried for a layer with nothing forced (make_conv2d_mfma_plan, and chain rule K under SNNHIP_CAT_KERNEL=auto)
bool conv2d_wide_is_default() {
    const char* w = snnhip::option("SNNHIP_CONV_WIDE");
    return !snnhip::option("SNNHIP_CONV") && !(w && atoi(w) == 0) && !snnhip::option("SNNHIP_CONV_BN") && !snnhip::option("SNNHIP_CONV_SPLITK") && !snnhip::option("SNNHIP_CONV_C8");
}

// fp16 3x3 stride-1 layers with IC % 16 == 0, OC % 32 == 0 and at least 0.75 blocks of 256 / 512 pixels per CU; SNNHIP_CONV=wide forces it for
// every eligible shape, SNNHIP_CONV_WIDE=0 keeps the 128-pixel kernel
int make_conv2d_wide_plan(snnhip_ctx* ctx, const ConvGeom& g, const float* w_oihw, const std::vector<float>& epi4, snnhip_plan** out) {
    if (g.dtype != SNNHIP_F16 || g.kh != 3 || g.kw != 3 || g.sh != 1 || g.sw != 1) return SNNHIP_E_UNSUPPORTED;
    if (g.IC % 16 != 0 || g.OC % 32 != 0 || g.act == SNNHIP_ACT_SILU_QUIRK) return SNNHIP_E_UNSUPPORTED;
    if (g.normShift && !act_is_simple(g.normAct)) return SNNHIP_E_UNSUPPORTED; // graph rule I: the branch-free activations only
    // chain rule K (g.C0 > 0): a plain concat of two tensors at the convolution's extent, whole 16-channel chunks in each; no upsampling on input 0, no fused
    // Pad, no norm in the staging, no residual (a third input)
    const bool cat = g.C0 > 0;
    if (cat && (g.C0 >= g.IC || g.C0 % 16 != 0 || g.catUp || g.preMode || g.normShift || g.addAct >= 0)) return SNNHIP_E_UNSUPPORTED;
    const double inCount = static_cast<double>(g.N) * (g.preMode ? g.srcH : g.H) * (g.preMode ? g.srcW : g.W) * g.IC; // (CAT: bounds each source's own offsets too)
    const double outCount = static_cast<double>(g.N) * g.OH * g.OW * g.OC;
    if (inCount >= 2147483647.0 || outCount >= 2147483647.0) return SNNHIP_E_UNSUPPORTED;
    const char* force = snnhip::option("SNNHIP_CONV");
    const char* catWord = snnhip::option("SNNHIP_CAT_KERNEL");
    // chain rule L (g.poolOH > 0), under the gates of conv2d_mfma's pooling form: the simple epilogue, one plain source, no residual, norm, fused Pad or
    // upsampling, and a pooled extent whose every window has its first position inside the output; the persistent form below has no pooling epilogue
    const bool pool = g.poolOH > 0;
    if (pool && (!act_is_simple(g.act) || g.addAct >= 0 || g.normShift || g.preMode || cat || g.poolOW <= 0 || 2 * g.poolOH > g.OH + 1 || 2 * g.poolOW > g.OW + 1)) return SNNHIP_E_UNSUPPORTED;
    const char* poolWord = snnhip::option("SNNHIP_POOL_KERNEL");
    const bool forced = (force && strcmp(force, "wide") == 0) || (cat && catWord && strcmp(catWord, "wide") == 0) ||
                        (pool && poolWord && strcmp(poolWord, "wide") == 0); // (the rule's named kernel: the size gate is skipped)
    // the 128 -> 128 body layers of the style graphs: the persistent form (conv2d_widep_f16.hip), unless it declines or SNNHIP_WIDE_PERSIST=0
    if (!pool && make_conv2d_widep_plan(ctx, g, w_oihw, epi4, out) == SNNHIP_OK) return SNNHIP_OK;

    // block shape: 256 px x 128 oc when the channels fill it, else 512 px x 64 / 32 oc
    int WM = 4, NT = 2, BN = 64;
    if (g.OC % 128 == 0) { WM = 2; NT = 2; BN = 128; }
    else if (g.OC % 64 != 0) { NT = 1; BN = 32; }
    if (const char* e = snnhip::option("SNNHIP_WIDE_BN")) { // experiments
        const int v = atoi(e);
        if (v == 128 && g.OC % 128 == 0) { WM = 2; NT = 2; BN = 128; }
        if (v == 64 && g.OC % 64 == 0) { WM = 4; NT = 2; BN = 64; }
        if (v == 32) { WM = 4; NT = 1; BN = 32; }
    }
    const int THs = WM == 2 ? 3 : 4, TH = 1 << THs, TW = 32;
    const int C8 = (WM == 2 && g.IC % 32 == 0 && g.C0 % 32 == 0) ? 2 : 1; // (CAT: a 32-channel chunk must not straddle the two sources -- the 16-channel chunk then)
    const int cus = ctx->props.multiProcessorCount > 0 ? ctx->props.multiProcessorCount : 256;
    const long tiles = static_cast<long>(g.N) * up_div(g.OH, TH) * up_div(g.OW, TW);
    // measured down to one 183x323 image (230 blocks of 256 pixels on 256 CUs): 24 us here, 35 us with the 128-pixel blocks; below that the
    // narrow blocks (and their split-K) fill the chip better
    if (!forced && tiles * (g.OC / BN) * 4 < 3L * cus) return SNNHIP_E_UNSUPPORTED;

    WideParams p{};
    p.N = g.N; p.H = g.H; p.W = g.W; p.IC = g.IC; p.OC = g.OC; p.padx = g.padx; p.pady = g.pady; p.padMode = g.padMode; p.useBN = g.useBN;
    p.OH = g.OH; p.OW = g.OW; p.THs = THs;
    p.tileH = TH + 2; p.tileW = TW + 2;
    p.tilesX = up_div(g.OW, TW); p.tilesY = up_div(g.OH, TH);
    p.nChunks = g.IC / (16 * C8);
    p.OCp = g.OC;
    p.total = p.tileH * p.tileW * (2 * C8 + 1); // 16-byte slots: Q of data + 1 of padding per pixel
    const int R = up_div(p.total, 256);
    p.bufFloats = R * 256 * 4; // every DMA lane has a slot
    p.zeroOfs = static_cast<int>((static_cast<size_t>(p.nChunks) * 9 * C8 + 3) * 2 * g.OC); // the last of the 4 zero steps behind the weights
    p.preMode = g.preMode; p.preX = g.preX; p.preY = g.preY; p.preShift = g.preMode ? g.preShift : 0;
    p.srcH = g.preMode ? g.srcH : g.H;
    p.srcW = g.preMode ? g.srcW : g.W;
    p.magicW = static_cast<unsigned>((0x100000000ull + static_cast<unsigned>(p.tileW) - 1) / static_cast<unsigned>(p.tileW));
    p.res = nullptr;
    p.ac2 = make_act_cfg(g.addAct >= 0 ? g.addAct : SNNHIP_ACT_NONE, g.addLeaky);

    const bool simple = act_is_simple(g.act);
    const bool withRes = g.addAct >= 0;
    if (withRes && !act_is_simple(g.addAct)) return SNNHIP_E_UNSUPPORTED; // (no graph of the zoo has one)
    WideFn fn = nullptr;
    if (WM == 2 && C8 == 2 && R <= 7) fn = pick_wide<2, 2, 2, 2, 7>(simple, withRes);
    if (WM == 2 && C8 == 1 && R <= 4) fn = pick_wide<2, 2, 2, 1, 4>(simple, withRes);
    if (WM == 4 && NT == 2 && R <= 8) fn = pick_wide<4, 1, 2, 1, 8>(simple, withRes);
    if (WM == 4 && NT == 1 && R <= 8) fn = pick_wide<4, 1, 1, 1, 8>(simple, withRes);
    WideCatFn catFn = nullptr;
    if (cat) {
        if (WM == 2 && C8 == 2 && R <= 7) catFn = pick_wide_cat<2, 2, 2, 2, 7>(simple);
        if (WM == 2 && C8 == 1 && R <= 4) catFn = pick_wide_cat<2, 2, 2, 1, 4>(simple);
        if (WM == 4 && NT == 2 && R <= 8) catFn = pick_wide_cat<4, 1, 2, 1, 8>(simple);
        if (WM == 4 && NT == 1 && R <= 8) catFn = pick_wide_cat<4, 1, 1, 1, 8>(simple);
        if (!catFn) return SNNHIP_E_UNSUPPORTED;
    }
    WidePoolFn poolFn = nullptr;
    if (pool) {
        if (WM == 2 && C8 == 2 && R <= 7) poolFn = conv2d_wide_pool_kernel<2, 2, 2, 2, 7>;
        if (WM == 2 && C8 == 1 && R <= 4) poolFn = conv2d_wide_pool_kernel<2, 2, 2, 1, 4>;
        if (WM == 4 && NT == 2 && R <= 8) poolFn = conv2d_wide_pool_kernel<4, 1, 2, 1, 8>;
        if (WM == 4 && NT == 1 && R <= 8) poolFn = conv2d_wide_pool_kernel<4, 1, 1, 1, 8>;
        if (!poolFn) return SNNHIP_E_UNSUPPORTED;
    }
    if (!fn) return SNNHIP_E_UNSUPPORTED;
    const int PIX = 128 * WM;
    p.epiOfs = static_cast<int>(std::max(static_cast<size_t>(2) * p.bufFloats * 4, static_cast<size_t>(PIX) * (BN + 8) * 2) / 4);
    const size_t lds = static_cast<size_t>(p.epiOfs) * 4 + static_cast<size_t>(BN) * 20 + (32 + 40) * sizeof(int) + // + the row / column tables of the staging
                       (g.normShift ? static_cast<size_t>(2) * g.IC * sizeof(float) : 0);                                  // + the norm's shift / mul (rule I)
    p.normShift = g.normShift;
    p.normMul = g.normMul;
    p.normAc = make_act_cfg(g.normShift ? g.normAct : SNNHIP_ACT_NONE, g.normLeaky);
    if (lds > 80 * 1024) return SNNHIP_E_UNSUPPORTED;

    auto* plan = new WideConvPlan();
    plan->ctx = ctx;
    plan->g = g;
    plan->w_oihw.assign(w_oihw, w_oihw + static_cast<size_t>(g.OC) * g.IC * 9);
    plan->epi4 = epi4;
    plan->p = p;
    plan->ac = make_act_cfg(g.act, g.leaky);
    plan->kernel = fn;
    plan->catKernel = catFn;
    plan->cp.C0 = g.C0;
    plan->poolKernel = poolFn;
    plan->pq.poolOH = g.poolOH;
    plan->pq.poolOW = g.poolOW;
#ifdef SNNHIP_WIDE_LDS_PAD_KB // experiment builds (tools/exp_one.sh): extra LDS per block = fewer blocks per CU (what does a block do when it has the CU to itself?)
    plan->ldsBytes = lds + static_cast<size_t>(SNNHIP_WIDE_LDS_PAD_KB) * 1024;
    hipFuncSetAttribute(reinterpret_cast<const void*>(plan->kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(plan->ldsBytes));
#else
    plan->ldsBytes = lds;
#endif
    plan->fusedAdd = g.addAct >= 0;
    if (plan->fusedAdd) plan->numInputs = 2;
    plan->grid = dim3(static_cast<unsigned>(tiles), g.OC / BN, 1);
    if (lds > 64 * 1024 && hipFuncSetAttribute(pool ? reinterpret_cast<const void*>(poolFn) : cat ? reinterpret_cast<const void*>(catFn) : reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)) != hipSuccess) {
        set_error("conv2d_wide: hipFuncSetAttribute(%zu) failed", lds);
        delete plan;
        return SNNHIP_E_HIP;
    }

    // weights: Wp[chunk][tap][c8][h][OC] x 8 halfs, ic = chunk*16*C8 + (c8*2 + h)*8 + j  (+ 10 zero steps: the ring's read-ahead, D <= 9, and the DMA's block of zeros)
    const size_t steps = static_cast<size_t>(p.nChunks) * 9 * C8;
    std::vector<float> wpk((steps + 10) * 2 * g.OC * 4, 0.0f); // the ring reads up to D = 9 steps past the last one
    _Float16* wph = reinterpret_cast<_Float16*>(wpk.data());
    for (int chunk = 0; chunk < p.nChunks; ++chunk)
        for (int t = 0; t < 9; ++t)
            for (int c8 = 0; c8 < C8; ++c8)
                for (int hh = 0; hh < 2; ++hh)
                    for (int j = 0; j < 8; ++j) {
                        const int ic = chunk * 16 * C8 + (c8 * 2 + hh) * 8 + j;
                        const size_t base = (((static_cast<size_t>(chunk) * 9 + t) * C8 + c8) * 2 + hh) * g.OC;
                        for (int o = 0; o < g.OC; ++o) wph[(base + o) * 8 + j] = static_cast<_Float16>(w_oihw[(static_cast<size_t>(o) * g.IC + ic) * 9 + t]);
                    }
    std::vector<float> epiP(static_cast<size_t>(g.OC) * 4, 0.0f);
    std::memcpy(epiP.data(), epi4.data(), sizeof(float) * 4 * static_cast<size_t>(g.OC));
    int rc = plan->upload(wpk.data(), wpk.size(), &plan->d_w);
    if (rc == SNNHIP_OK) rc = plan->upload(epiP.data(), epiP.size(), &plan->d_epi);
    if (rc != SNNHIP_OK) {
        delete plan;
        return rc;
    }
    // K-loop token: where a CU holds exactly two of these blocks and the grid is several rounds of them (SNNHIP_WIDE_TOKEN=0 / 1 forces it off / on)
    {
        const char* tk = snnhip::option("SNNHIP_WIDE_TOKEN");
        const bool twoPerCu = lds > 53 * 1024;
        const bool want = tk ? atoi(tk) != 0 : false;
        if (want && twoPerCu) {
            void* buf = nullptr;
            if (snnhip::dev_malloc(&buf, kTokSlots * sizeof(unsigned)) == hipSuccess) {
                plan->deviceAllocs.push_back(buf);
                if (hipMemset(buf, 0, kTokSlots * sizeof(unsigned)) == hipSuccess) plan->p.kTok = static_cast<unsigned*>(buf);
            }
        }
    }
    plan->inDims[0] = g.N; plan->inDims[1] = p.srcH; plan->inDims[2] = p.srcW; plan->inDims[3] = g.IC;
    plan->outDims[0] = g.N; plan->outDims[1] = g.OH; plan->outDims[2] = g.OW; plan->outDims[3] = g.OC;
    plan->dtype = SNNHIP_F16;
    plan->flops = 2.0 * 9 * g.IC * g.OC * static_cast<double>(g.OH) * g.OW * g.N;
    plan->bytes = 2.0 * (static_cast<double>(g.N) * p.srcH * p.srcW * g.IC + static_cast<double>(g.N) * g.OH * g.OW * g.OC + static_cast<double>(g.OC) * g.IC * 9);
    char buf[256];
    snprintf(buf, sizeof(buf), "conv2d_mfma_wide_f16_32x32x16 k=3x3 s=1 ic=%d oc=%d tile=%dx32px x %doc (4x%d MFMA tiles per wave) chunk=%d lds=%zuB", g.IC, g.OC, TH, BN, NT,
             16 * C8, lds);
    plan->desc = buf;
    if (cat) { // two inputs; inDims describes input 0, the bytes count both once (their sum is the term above)
        plan->numInputs = 2;
        plan->inDims[3] = g.C0;
        plan->desc += " +concat(" + std::to_string(g.C0) + "+" + std::to_string(g.IC - g.C0) + ")";
    }
    if (pool) { // the input, the weights and the POOLED output: the full-resolution tensor never exists
        plan->outDims[1] = g.poolOH;
        plan->outDims[2] = g.poolOW;
        plan->bytes = 2.0 * (static_cast<double>(g.N) * g.H * g.W * g.IC + static_cast<double>(g.N) * g.poolOH * g.poolOW * g.OC + static_cast<double>(g.OC) * g.IC * 9);
        plan->desc += " +maxpool(2x2)";
    }
    if (g.preMode) plan->desc += " +pad(" + std::string(g.preMode == SNNHIP_PAD_REFLECT ? "reflect" : g.preMode == SNNHIP_PAD_REPLICATE ? "replicate" : "constant") + ")";
    if (g.preMode && g.preShift) plan->desc += " +upsample(x2)";
    if (g.normShift) plan->desc = "instancenorm(act=" + std::to_string(g.normAct) + ", in LDS behind the DMA) -> " + plan->desc;
    if (plan->fusedAdd) {
        plan->desc += " +add";
        plan->bytes += 2.0 * static_cast<double>(g.N) * g.OH * g.OW * g.OC;
    }
    if (plan->p.kTok) plan->desc += " +ktoken";
    *out = plan;
    return SNNHIP_OK;
}

} // namespace snnhip
