// conv2d_wino.hip -- fp32 3x3 stride-1 convolution as Winograd F(2x2,3x3) on the gfx950 matrix cores (v_mfma_f32_16x16x4_f32), for the
// GEMM-shaped 3x3 layers of the reference's Conv2D operator: the ResNet-18 body (BASELINE configs[2]), U-Net, YOLO.
//
// Same operator contract as conv2d_mfma.hip / conv2d_generic.hip (shadertemplate_vk_conv2d.comp:148-347: zero padding by clipped
// taps, bias -> BN -> activation epilogue, optional fused residual Add of chain rule E); only the evaluation differs:
//     Y = At [ sum_ic (G g Gt) .* (Bt d B) ] A          per 2x2 output tile, 16 "positions" per tile
// which needs 16 multiplies per 2x2 tile, channel pair instead of 36 -- the matrix pipe does 2.25x fewer flops than the direct implicit
// GEMM.  fp32 MFMA and the fp32 VALU share the FMA lanes on this chip (tools/ubench_issue.hip), so the transforms are kept to the
// minimum: activations are only added / subtracted (Bt, At have entries 0, +-1), G g Gt is computed on the host in double.
//
// Work decomposition (default: one block = 256 threads = 4 waves, two blocks per CU; SNNHIP_WINO_OPB=2: 512 threads / 64 channels, one per CU):
//   block tile = 64 Winograd tiles (TB images x TTH x TTW tiles = TB x 2TTH x 2TTW output pixels) x 32 output channels
//   wave tg: tile group = 16 consecutive tiles (the N of the MFMA) x 2 blocks of 16 channels (the M)
//   K loop over 8-channel chunks, double-buffered in LDS, one barrier per chunk:
//     U slab   [16 positions][2 channel pairs][lane = (k, m)] float4 = the MFMA A operands of both K steps and both channel blocks of a wave,
//              pre-packed on the host in exactly this order (a chunk's slab is 32 KB of contiguous global memory; a lane's read is
//              base + 16*lane: conflict-free ds_read_b128)
//     input    4 channel-pair planes [image][row][col] float2 of the (2TTH+2) x (2TTW+2) halo tile; plane pitch = 0 mod 64 floats and row
//              pitch = TTW mod 16 pixels make the ds_read_b128 of two adjacent patch pixels conflict-free across the wave's 16 tiles x 4
//              pairs (lane groups {0-3,12-15,20-27} ...: MI355X_MICROARCH.md, LDS)
//     per chunk and wave: 8 ds_read_b128 (its 4x4 patch: lane = (tile n, channel pair k)), Bt d B on the VALU (64 adds), then
//     2 K steps x 16 positions x 2 channel blocks = 64 MFMAs whose B operand is the transform result straight from registers (the
//     transformed tile never goes through LDS) and whose A operands are one ds_read_b128 per position
//   accumulators: 16 positions x 2 blocks x 4 = 128 registers; At M A on the VALU once per tile, epilogue, 16-byte channel-contiguous stores
//   split-K over blockIdx.z (raw partial sums to a workspace + the reduce/epilogue pass of conv2d_mfma.hip) when a layer has too few
//   block tiles to fill 256 CUs (ResNet's 14x14 / 7x7 stages).
#include <cstring>
#include <vector>

#include "epilogue.h"
#include "snnhip_internal.h"

#ifndef SNNHIP_WINO_ABL
#define SNNHIP_WINO_ABL 0 // ablation builds only (tools/ablate_wino.sh; results are wrong by construction): 1 no barrier in the chunk loop,
#endif                    // 2 no LDS stores, 4 no global loads, 8 no input transform, 16 no U reads, 32 no patch reads, 64 no U DMA, 128 no activation loads

namespace snnhip {

// conv2d_mfma.hip: the split-K reduce / epilogue pass
int launch_splitk_reduce(snnhip_ctx* ctx, int OC, int splitK, int useBN, const ActCfg& ac, const float* ws, const float4* e4, snnhip_tensor* out,
                         const snnhip_tensor* res, const ActCfg& ac2);
// ... and its pooling form (chain rule L): ws = [splitK][N][OH][OW][OC] raw sums -> out = maxpool2x2(act(BN(bias + sum_z ws[z]))), [N][out->h][out->w][OC]
int launch_splitk_reduce_pool(snnhip_ctx* ctx, int OH, int OW, int splitK, int useBN, const ActCfg& ac, const float* ws, const float4* e4, snnhip_tensor* out);

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct WinoParams {
    int N, H, W, IC, OC, OH, OW, padx, pady;
    int TBs, TTHs, TTWs;   // log2: images, tile rows, tile columns of a block tile (TB * TTH * TTW = 64 tiles)
    int tilesX, tilesY;    // block tiles along x / y
    int inH, inW;          // staged halo tile per image: 2*TTH + 2, 2*TTW + 2 pixels
    int rowPitch;          // pixels per staged row
    int planeStride;       // floats between the channel-pair planes
    int total;             // float4 elements staged per chunk (TB * inH * inW * 2)
    int bufFloats;         // floats per LDS buffer (U slab + 4 planes)
    int nChunks, splitK, chunksPerSplit;
    int OCblocks;          // ceil(OC / (32 * OPB))
    int useBN;
    const float* res;      // fused residual Add (chain rule E), or nullptr
    ActCfg ac2;
};

// OPB = output-channel pairs (2 x 16 channels) per block: 2 -> 512 threads, 64 channels, one block per CU; 1 -> 256 threads, 32 channels,
// two independent blocks per CU (their barriers and LDS-read bursts drift apart, the pair of waves on a SIMD is no longer in lock step)
// KS = 2 (round 6; OPB = 1 only): the block's channel chunks are split over TWO groups of four waves -- each group stages its own chunks into its own
// pair of LDS buffers and runs the K loop below on them, barrier for barrier --, then the groups exchange half of their sums through LDS (group g keeps
// output-channel block g: it hands the partner the other block's sixteen positions and adds the partner's to its own -- p0 + p1 in both groups, the order
// of the reduce pass), and every wave runs the epilogue of ONE channel block.  What a 14x14 stage needed split-K over blockIdx.z + a reduce launch for
// (partial sums through HBM, 6 us per launch) stays inside the block.
// CAT (chain rule K: Concatenate -> Conv2D, conv2d_wino_cat_kernel below): the K chunks come from TWO tensors.  A chunk is 8 channels and C0 a multiple of 8,
// so a chunk lies wholly in one source and a K range (a block's, a blockIdx.z slice's, a K group's) changes source at most once: the source is
// block-uniform state -- base pointer and channel origin in scalar registers, the threads' global offsets taken again from that source's own pitch and
// extent at the one chunk where it changes (set in the prologue from the range's first chunk).  One offset set is live, as in the single-source form.
struct WinoCatParams {
    const float* x1;   // input 1: N x H x W x pitch1
    int c0Chunks;      // chunks [0, c0Chunks) are input 0's
    int pitch0, pitch1; // channels (= pixel pitch) of the two inputs
    int srcH, srcW;    // input 0's own extent: H x W, or the low-resolution one behind the nearest x2 upsampling ...
    int shift0;        // ... whose pixel of (sy, sx) is (sy >> shift0, sx >> shift0); input 1 is always at H x W
};

// POOL (chain rule L: Conv2D -> MaxPooling2D 2x2 stride 2, conv2d_wino_pool_kernel below): a lane's F(2x2,3x3) output tile starts at an even row and column, so it
// IS one pooling window -- the epilogue takes the maximum of the lane's four finished values and stores one pixel of [N][poolOH][poolOW][OC] (conv2d_wino_body.h).
struct WinoPoolParams {
    int poolOH, poolOW; // the pooling plan's own output extent: ceil or floor of OH / 2, OW / 2
};

template <bool SIMPLE, int OPB, int KS = 1>
__global__ __launch_bounds__(256 * OPB * KS, KS > 1 ? 1 : 3 - OPB) void conv2d_wino_kernel(WinoParams p, ActCfg ac, const float* __restrict__ x, const float4* __restrict__ ug,
                                                                        const float4* __restrict__ epi, float* __restrict__ y, float* __restrict__ ws) {
    constexpr bool CAT = false, POOL = false;
    const WinoCatParams cp = {};
    const WinoPoolParams pq = {};
#include "conv2d_wino_body.h"
}

// chain rule K: x = input 0 (cp.pitch0 channels, cp.srcH x cp.srcW), cp.x1 = input 1; the weight image is the layer's own, K in concatenated channel order
template <bool SIMPLE, int OPB, int KS = 1>
__global__ __launch_bounds__(256 * OPB * KS, KS > 1 ? 1 : 3 - OPB) void conv2d_wino_cat_kernel(WinoParams p, WinoCatParams cp, ActCfg ac, const float* __restrict__ x,
                                                                            const float4* __restrict__ ug, const float4* __restrict__ epi, float* __restrict__ y,
                                                                            float* __restrict__ ws) {
    constexpr bool CAT = true, POOL = false;
    const WinoPoolParams pq = {};
#include "conv2d_wino_body.h"
}

// chain rule L: y is the POOLED tensor [N][pq.poolOH][pq.poolOW][OC] (splitK == 1) -- or nobody's: the raw partial tiles go to ws at full resolution
template <bool SIMPLE, int OPB, int KS = 1>
__global__ __launch_bounds__(256 * OPB * KS, KS > 1 ? 1 : 3 - OPB) void conv2d_wino_pool_kernel(WinoParams p, WinoPoolParams pq, ActCfg ac, const float* __restrict__ x,
                                                                             const float4* __restrict__ ug, const float4* __restrict__ epi, float* __restrict__ y,
                                                                             float* __restrict__ ws) {
    constexpr bool CAT = false, POOL = true;
    const WinoCatParams cp = {};
#include "conv2d_wino_body.h"
}

typedef void (*WinoCatFn)(WinoParams, WinoCatParams, ActCfg, const float*, const float4*, const float4*, float*, float*);
template <bool SIMPLE>
WinoCatFn pick_wino_cat(int opb, int ks) {
    return ks == 2 ? conv2d_wino_cat_kernel<SIMPLE, 1, 2> : opb == 2 ? conv2d_wino_cat_kernel<SIMPLE, 2> : conv2d_wino_cat_kernel<SIMPLE, 1>;
}

typedef void (*WinoPoolFn)(WinoParams, WinoPoolParams, ActCfg, const float*, const float4*, const float4*, float*, float*);
WinoPoolFn pick_wino_pool(int opb, int ks) { // (the rule takes the simple activations only)
    return ks == 2 ? conv2d_wino_pool_kernel<true, 1, 2> : opb == 2 ? conv2d_wino_pool_kernel<true, 2> : conv2d_wino_pool_kernel<true, 1>;
}

struct WinoConvPlan : ConvPlanBase {
    WinoParams p;
    ActCfg ac;
    float* d_u = nullptr;
    float* d_epi = nullptr;
    float* d_ws = nullptr;
    size_t ldsBytes = 0;
    dim3 grid;
    bool fusedAdd = false;
    bool simple = true;
    int opb = 1;
    int ks = 1; // K groups per block (2: eight waves, the channel chunks split inside the block)
    WinoCatParams cp = {}; // chain rule K (g.C0 > 0): two inputs in the concat's order
    WinoCatFn catKernel = nullptr;
    WinoPoolParams pq = {}; // chain rule L (g.poolOH > 0): the output is the pooled tensor
    WinoPoolFn poolKernel = nullptr;

    int run_pool(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) {
        SNNHIP_REQUIRE(nIn == 1, "conv2d+maxpool: expects 1 input, got %d", nIn);
        const snnhip_tensor* x = in[0];
        SNNHIP_REQUIRE(x->n == p.N && x->h == p.H && x->w == p.W && x->c == p.IC && x->dtype == SNNHIP_F32, "conv2d+maxpool: input dims %dx%dx%dx%d (dtype %d) != plan %dx%dx%dx%d fp32",
                       x->n, x->h, x->w, x->c, x->dtype, p.N, p.H, p.W, p.IC);
        SNNHIP_REQUIRE(out->n == p.N && out->h == pq.poolOH && out->w == pq.poolOW && out->c == p.OC && out->dtype == SNNHIP_F32,
                       "conv2d+maxpool: output dims %dx%dx%dx%d (dtype %d) != plan %dx%dx%dx%d fp32", out->n, out->h, out->w, out->c, out->dtype, p.N, pq.poolOH, pq.poolOW, p.OC);
        const float4* e4 = reinterpret_cast<const float4*>(d_epi);
        SNNHIP_LAUNCH(poolKernel, grid, dim3(256 * opb * ks), ldsBytes, ctx->stream, p, pq, ac, x->data, reinterpret_cast<const float4*>(d_u), e4, out->data, d_ws);
        SNNHIP_CHECK_HIP(hipGetLastError());
        if (p.splitK > 1) return launch_splitk_reduce_pool(ctx, p.OH, p.OW, p.splitK, p.useBN, ac, d_ws, e4, out);
        return SNNHIP_OK;
    }

    int run_cat(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) {
        SNNHIP_REQUIRE(nIn == 2, "conv2d+concat: expects 2 inputs, got %d", nIn);
        const snnhip_tensor *x0 = in[0], *x1 = in[1];
        SNNHIP_REQUIRE(x0->n == p.N && x0->h == cp.srcH && x0->w == cp.srcW && x0->c == cp.pitch0 && x0->dtype == SNNHIP_F32,
                       "conv2d+concat: input 0 dims %dx%dx%dx%d (dtype %d) != plan %dx%dx%dx%d fp32", x0->n, x0->h, x0->w, x0->c, x0->dtype, p.N, cp.srcH, cp.srcW, cp.pitch0);
        SNNHIP_REQUIRE(x1->n == p.N && x1->h == p.H && x1->w == p.W && x1->c == cp.pitch1 && x1->dtype == SNNHIP_F32,
                       "conv2d+concat: input 1 dims %dx%dx%dx%d (dtype %d) != plan %dx%dx%dx%d fp32", x1->n, x1->h, x1->w, x1->c, x1->dtype, p.N, p.H, p.W, cp.pitch1);
        SNNHIP_REQUIRE(out->n == p.N && out->h == p.OH && out->w == p.OW && out->c == p.OC && out->dtype == SNNHIP_F32, "conv2d: output dims %dx%dx%dx%d != plan %dx%dx%dx%d",
                       out->n, out->h, out->w, out->c, p.N, p.OH, p.OW, p.OC);
        WinoCatParams c = cp; // per-launch copy: input 1's pointer travels in the kernel argument block
        c.x1 = x1->data;
        const float4* e4 = reinterpret_cast<const float4*>(d_epi);
        SNNHIP_LAUNCH(catKernel, grid, dim3(256 * opb * ks), ldsBytes, ctx->stream, p, c, ac, x0->data, reinterpret_cast<const float4*>(d_u), e4, out->data, d_ws);
        SNNHIP_CHECK_HIP(hipGetLastError());
        if (p.splitK > 1) return launch_splitk_reduce(ctx, p.OC, p.splitK, p.useBN, ac, d_ws, e4, out, nullptr, p.ac2);
        return SNNHIP_OK;
    }

    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        if (catKernel) return run_cat(in, nIn, out);
        if (poolKernel) return run_pool(in, nIn, out);
        SNNHIP_REQUIRE(nIn == (fusedAdd ? 2 : 1), "conv2d: expects %d input(s), got %d", fusedAdd ? 2 : 1, nIn);
        const snnhip_tensor* x = in[0];
        WinoParams q = p; // per-launch copy: the residual pointer travels in the kernel argument block
        q.res = nullptr;
        if (fusedAdd) {
            const snnhip_tensor* r = in[1];
            SNNHIP_REQUIRE(r->n == p.N && r->h == p.OH && r->w == p.OW && r->c == p.OC && r->dtype == dtype,
                           "conv2d+add: residual %dx%dx%dx%d (dtype %d) does not match the output %dx%dx%dx%d", r->n, r->h, r->w, r->c, r->dtype, p.N, p.OH,
                           p.OW, p.OC);
            q.res = p.splitK > 1 ? nullptr : r->data; // split-K: the reduce pass adds it
        }
        SNNHIP_REQUIRE(x->n == p.N && x->h == p.H && x->w == p.W && x->c == p.IC, "conv2d: input dims %dx%dx%dx%d != plan %dx%dx%dx%d", x->n, x->h, x->w,
                       x->c, p.N, p.H, p.W, p.IC);
        SNNHIP_REQUIRE(out->n == p.N && out->h == p.OH && out->w == p.OW && out->c == p.OC, "conv2d: output dims %dx%dx%dx%d != plan %dx%dx%dx%d", out->n,
                       out->h, out->w, out->c, p.N, p.OH, p.OW, p.OC);
        const float4* u4 = reinterpret_cast<const float4*>(d_u);
        const float4* e4 = reinterpret_cast<const float4*>(d_epi);
        if (ks == 2) {
            if (simple) SNNHIP_LAUNCH((conv2d_wino_kernel<true, 1, 2>), grid, dim3(512), ldsBytes, ctx->stream, q, ac, x->data, u4, e4, out->data, d_ws);
            else SNNHIP_LAUNCH((conv2d_wino_kernel<false, 1, 2>), grid, dim3(512), ldsBytes, ctx->stream, q, ac, x->data, u4, e4, out->data, d_ws);
        } else if (opb == 2) {
            if (simple) SNNHIP_LAUNCH((conv2d_wino_kernel<true, 2>), grid, dim3(512), ldsBytes, ctx->stream, q, ac, x->data, u4, e4, out->data, d_ws);
            else SNNHIP_LAUNCH((conv2d_wino_kernel<false, 2>), grid, dim3(512), ldsBytes, ctx->stream, q, ac, x->data, u4, e4, out->data, d_ws);
        } else {
            if (simple) SNNHIP_LAUNCH((conv2d_wino_kernel<true, 1>), grid, dim3(256), ldsBytes, ctx->stream, q, ac, x->data, u4, e4, out->data, d_ws);
            else SNNHIP_LAUNCH((conv2d_wino_kernel<false, 1>), grid, dim3(256), ldsBytes, ctx->stream, q, ac, x->data, u4, e4, out->data, d_ws);
        }
        SNNHIP_CHECK_HIP(hipGetLastError());
        if (p.splitK > 1) return launch_splitk_reduce(ctx, p.OC, p.splitK, p.useBN, ac, d_ws, e4, out, fusedAdd ? in[1] : nullptr, p.ac2);
        return SNNHIP_OK;
    }
};

} // namespace

// where this kernel is a layer's own plan with nothing forced (make_conv2d_mfma_plan, and chain rule K under SNNHIP_CAT_KERNEL=auto): GEMM-sized channel
// counts, no norm in the staging, no switch that pins another kernel or a block shape
bool conv2d_wino_is_default(const ConvGeom& g) {
    const char* w = snnhip::option("SNNHIP_CONV_WINO");
    return !snnhip::option("SNNHIP_CONV") && !(w && atoi(w) == 0) && !snnhip::option("SNNHIP_CONV_BN") && !snnhip::option("SNNHIP_CONV_C8") && g.IC >= 32 && g.OC >= 32 && !g.normShift;
}

int make_conv2d_wino_plan(snnhip_ctx* ctx, const ConvGeom& g, const float* w_oihw, const std::vector<float>& epi4, snnhip_plan** out) {
    // eligibility: fp32, 3x3, stride 1, zero padding (or none), no fused Pad in front, whole 8-channel chunks and 16-channel output blocks
    // chain rule K (g.C0 > 0): two sources, whole chunks in each, no third input (fused Add), no norm in the staging; input 0 alone may sit behind a
    // nearest x2 upsampling (catUp: the identity pad + shift of rule D, srcH x srcW its low-resolution extent) -- every other fused Pad stays refused
    const bool cat = g.C0 > 0;
    const bool catUp = cat && g.catUp && g.preMode == SNNHIP_PAD_CONSTANT && g.preX == 0 && g.preY == 0 && g.preShift == 1 && g.H == 2 * g.srcH && g.W == 2 * g.srcW;
    if (g.dtype != SNNHIP_F32 || g.kh != 3 || g.kw != 3 || g.sh != 1 || g.sw != 1 || (g.preMode != 0 && !catUp) || (g.catUp && !catUp)) return SNNHIP_E_UNSUPPORTED;
    if (g.padMode != SNNHIP_PAD_CONSTANT && g.padMode != SNNHIP_PAD_NONE) return SNNHIP_E_UNSUPPORTED;
    if (g.IC % 8 != 0 || g.OC % 16 != 0 || g.act == SNNHIP_ACT_SILU_QUIRK) return SNNHIP_E_UNSUPPORTED;
    if (cat && (g.C0 >= g.IC || g.C0 % 8 != 0 || g.addAct >= 0 || g.normShift)) return SNNHIP_E_UNSUPPORTED;
    // chain rule L (g.poolOH > 0), under the gates of conv2d_mfma's pooling form: the simple epilogue, one plain source, no third input, and a pooled extent whose
    // every window has its first position inside the convolution's output (the ceil or the floor of half of it)
    const bool pool = g.poolOH > 0;
    if (pool && (!act_is_simple(g.act) || g.addAct >= 0 || g.normShift || g.preMode || cat || g.poolOW <= 0 || 2 * g.poolOH > g.OH + 1 || 2 * g.poolOW > g.OW + 1)) return SNNHIP_E_UNSUPPORTED;
    const int srcH0 = catUp ? g.srcH : g.H, srcW0 = catUp ? g.srcW : g.W;
    // 32-bit element offsets in the staging path: each source on its own
    const double inCount = cat ? std::max(static_cast<double>(g.N) * srcH0 * srcW0 * g.C0, static_cast<double>(g.N) * g.H * g.W * (g.IC - g.C0)) : static_cast<double>(g.N) * g.H * g.W * g.IC;
    const double outCount = static_cast<double>(g.N) * g.OH * g.OW * g.OC;
    if (inCount >= 2147483647.0 || outCount >= 2147483647.0) return SNNHIP_E_UNSUPPORTED;

    // block tile: TB x TTH x TTW = 64 Winograd tiles, minimising padded tiles; a wave's 16 consecutive tiles must not straddle images
    // (TTH * TTW >= 16 and TTH >= 16 / TTW when TTW < 16: the bank analysis of the patch reads assumes whole tile rows of one image)
    const int tilesW = up_div(g.OW, 2), tilesH = up_div(g.OH, 2);
    // OPB = 1 (default): 256-thread blocks of 32 output channels, two per CU; SNNHIP_WINO_OPB=2: 512-thread blocks of 64 channels, one per CU
    int opb = 1;
    if (const char* e = snnhip::option("SNNHIP_WINO_OPB")) opb = atoi(e) == 2 ? 2 : 1;
    const int ocPerBlock = 32 * opb, kUFloats = 4096 * opb;
    int best[3] = {0, 2, 4};
    double bestCost = 1e300;
    for (int ws = 2; ws <= 5; ++ws)
        for (int hs = 0; hs + ws <= 6; ++hs) {
            const int TTW = 1 << ws, TTH = 1 << hs, TB = 64 / (TTW * TTH);
            if (TTW < 16 && TTH < 16 / TTW) continue;
            if (TB * (2 * TTH + 2) * (2 * TTW + 2) * 2 > 1024) continue; // two staged float4 per thread
            const double cost = static_cast<double>(up_div(g.N, TB)) * up_div(tilesH, TTH) * up_div(tilesW, TTW) * (1.0 + 0.02 * (2.0 / TTH + 2.0 / TTW));
            if (cost < bestCost) {
                bestCost = cost;
                best[0] = 6 - ws - hs;
                best[1] = hs;
                best[2] = ws;
            }
        }
    WinoParams p = {};
    p.N = g.N; p.H = g.H; p.W = g.W; p.IC = g.IC; p.OC = g.OC; p.OH = g.OH; p.OW = g.OW; p.padx = g.padx; p.pady = g.pady;
    p.TBs = best[0]; p.TTHs = best[1]; p.TTWs = best[2];
    const int TB = 1 << p.TBs, TTH = 1 << p.TTHs, TTW = 1 << p.TTWs;
    p.tilesX = up_div(tilesW, TTW);
    p.tilesY = up_div(tilesH, TTH);
    p.inH = 2 * TTH + 2;
    p.inW = 2 * TTW + 2;
    p.rowPitch = p.inW;
    // a wave's 16 tiles span 16 / TTW tile rows: their bank offsets (tile-row stride = 4 * rowPitch floats) must be distinct multiples of 4 * TTW
    // mod 64 -> rowPitch = 8 mod 16 for TTW = 8, an odd multiple of 4 for TTW = 4
    if (TTW == 8)
        while (p.rowPitch % 16 != 8) ++p.rowPitch;
    if (TTW == 4)
        while (p.rowPitch % 8 != 4) ++p.rowPitch;
    p.planeStride = round_up(TB * p.inH * p.rowPitch * 2, 64); // 0 mod 64 floats: with ds_read_b128's lane groups the k and k+1 planes interleave bank-exactly
    p.total = TB * p.inH * p.inW * 2;
    p.bufFloats = kUFloats + 4 * p.planeStride;
    p.nChunks = g.IC / 8;
    p.OCblocks = up_div(g.OC, ocPerBlock);
    p.useBN = g.useBN;
    p.ac2 = make_act_cfg(g.addAct >= 0 ? g.addAct : 0, g.addLeaky);
    const size_t lds = static_cast<size_t>(2) * p.bufFloats * sizeof(float);
    if (lds > 160 * 1024) return SNNHIP_E_UNSUPPORTED;

    // split-K: split the channel chunks while the layer has fewer block tiles than resident block slots
    const int cus = (ctx->props.multiProcessorCount > 0 ? ctx->props.multiProcessorCount : 256) * (3 - opb);
    const int blocks = p.tilesX * p.tilesY * up_div(g.N, TB) * p.OCblocks;
    int splitK = 1;
    if (const char* e = snnhip::option("SNNHIP_CONV_SPLITK")) splitK = std::max(1, atoi(e));
    else
        while (blocks * splitK * 2 <= cus && splitK * 2 <= p.nChunks / 2) splitK *= 2; // doubling must still fit one round of blocks
    splitK = std::min(splitK, p.nChunks);
    // round 6: the first factor of two of the split stays INSIDE the block (two K groups of four waves, kernel template KS = 2): 256 -> 256 @14x14 needs no
    // reduce launch at all, 512 -> 512 @7x7 reduces two partial tensors instead of four.  SNNHIP_WINO_KGROUPS=1 keeps the split over blockIdx.z only.
    int ks = 1;
    {
        const char* e = snnhip::option("SNNHIP_WINO_KGROUPS");
        const bool wanted = e ? atoi(e) == 2 : (splitK == 2 && !snnhip::option("SNNHIP_CONV_SPLITK")); // (where the reduce launch disappears; a deeper split keeps it)
        if (wanted && opb == 1 && splitK % 2 == 0 && p.nChunks % splitK == 0) {
            ks = 2;
            splitK /= 2;
        } else if (e && atoi(e) == 2 && opb == 1 && splitK == 1 && p.nChunks % 2 == 0) {
            ks = 2; // forced on a layer that would not split at all (tests)
        }
    }
    p.chunksPerSplit = up_div(p.nChunks, splitK);
    p.splitK = up_div(p.nChunks, p.chunksPerSplit);
    if (ks == 2 && (p.nChunks % p.splitK != 0 || p.chunksPerSplit % 2 != 0)) return SNNHIP_E_UNSUPPORTED; // (cannot happen with the conditions above)
    size_t ldsAll = ks == 2 ? std::max<size_t>(2 * lds, 128 * 1024) : lds; // two groups' buffers; the exchange of the sums needs 8 x 16 KB
    if (const char* padOpt = snnhip::option("SNNHIP_WINO_LDS_PAD")) ldsAll = std::min<size_t>(160 * 1024, ldsAll + static_cast<size_t>(atoi(padOpt))); // developer switch: residency experiments
    if (ldsAll > 160 * 1024) return SNNHIP_E_UNSUPPORTED;

    auto* plan = new WinoConvPlan();
    plan->ctx = ctx;
    plan->g = g;
    plan->w_oihw.assign(w_oihw, w_oihw + static_cast<size_t>(g.OC) * g.IC * 9);
    plan->epi4 = epi4;
    plan->p = p;
    plan->ac = make_act_cfg(g.act, g.leaky);
    plan->simple = act_is_simple(g.act);
    plan->ldsBytes = ldsAll;
    plan->ks = ks;
    plan->fusedAdd = g.addAct >= 0;
    if (plan->fusedAdd) plan->numInputs = 2;
    plan->opb = opb;
    plan->grid = dim3(p.tilesX * p.tilesY * up_div(g.N, TB), p.OCblocks, p.splitK);
    plan->dtype = SNNHIP_F32;
    if (cat) {
        plan->numInputs = 2;
        plan->cp.c0Chunks = g.C0 / 8;
        plan->cp.pitch0 = g.C0;
        plan->cp.pitch1 = g.IC - g.C0;
        plan->cp.srcH = srcH0;
        plan->cp.srcW = srcW0;
        plan->cp.shift0 = catUp ? 1 : 0;
        plan->catKernel = plan->simple ? pick_wino_cat<true>(opb, ks) : pick_wino_cat<false>(opb, ks);
        if (ldsAll > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(plan->catKernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(ldsAll)) != hipSuccess) {
            set_error("conv2d_wino: hipFuncSetAttribute(%zu) failed", ldsAll);
            delete plan;
            return SNNHIP_E_HIP;
        }
    }
    if (pool) {
        plan->pq.poolOH = g.poolOH;
        plan->pq.poolOW = g.poolOW;
        plan->poolKernel = pick_wino_pool(opb, ks);
        if (ldsAll > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(plan->poolKernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(ldsAll)) != hipSuccess) {
            set_error("conv2d_wino: hipFuncSetAttribute(%zu) failed", ldsAll);
            delete plan;
            return SNNHIP_E_HIP;
        }
    }
    for (int s = 0; s < 2 && !cat && !pool; ++s) {
        const void* fn = ks == 2 ? (s ? reinterpret_cast<const void*>(conv2d_wino_kernel<true, 1, 2>) : reinterpret_cast<const void*>(conv2d_wino_kernel<false, 1, 2>))
                         : opb == 2 ? (s ? reinterpret_cast<const void*>(conv2d_wino_kernel<true, 2>) : reinterpret_cast<const void*>(conv2d_wino_kernel<false, 2>))
                                  : (s ? reinterpret_cast<const void*>(conv2d_wino_kernel<true, 1>) : reinterpret_cast<const void*>(conv2d_wino_kernel<false, 1>));
        if (ldsAll > 64 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(ldsAll)) != hipSuccess) {
            set_error("conv2d_wino: hipFuncSetAttribute(%zu) failed", ldsAll);
            delete plan;
            return SNNHIP_E_HIP;
        }
    }
    if (p.splitK > 1) {
        void* wsp = nullptr;
        const size_t wsBytes = static_cast<size_t>(p.splitK) * g.N * g.OH * g.OW * g.OC * sizeof(float);
        if (snnhip::dev_malloc(&wsp, wsBytes) != hipSuccess) {
            set_error("conv2d_wino: split-K workspace of %zu bytes", wsBytes);
            delete plan;
            return SNNHIP_E_HIP;
        }
        plan->deviceAllocs.push_back(wsp);
        plan->d_ws = static_cast<float*>(wsp);
    }

    // U = G g Gt in double, G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]], packed as the kernel's LDS image:
    //   Ug[oc block of 64][chunk][pos = 4i + j][op][lane = 16k + m] float4 {ocb = 2 op: ic = 8 chunk + 2k, + 1; ocb = 2 op + 1: the same two}, oc = 64 block + 16 ocb + m
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    std::vector<float> U(static_cast<size_t>(p.OCblocks) * p.nChunks * kUFloats, 0.0f);
    for (int oc = 0; oc < g.OC; ++oc)
        for (int ic = 0; ic < g.IC; ++ic) {
            const float* w = w_oihw + (static_cast<size_t>(oc) * g.IC + ic) * 9;
            double Gg[4][3];
            for (int i = 0; i < 4; ++i)
                for (int b = 0; b < 3; ++b) Gg[i][b] = G[i][0] * w[0 * 3 + b] + G[i][1] * w[1 * 3 + b] + G[i][2] * w[2 * 3 + b];
            const int blk = oc / ocPerBlock, ocb = (oc % ocPerBlock) / 16, m = oc % 16, chunk = ic / 8, kk = (ic % 8) / 2, s = ic % 2;
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) {
                    const double u = Gg[i][0] * G[j][0] + Gg[i][1] * G[j][1] + Gg[i][2] * G[j][2];
                    const size_t at = ((static_cast<size_t>(blk) * p.nChunks + chunk) * 16 * opb + (i * 4 + j) * opb + (ocb >> 1)) * 256 + (kk * 16 + m) * 4 + (ocb & 1) * 2 + s;
                    U[at] = static_cast<float>(u);
                }
        }
    std::vector<float> epiP(static_cast<size_t>(p.OCblocks) * ocPerBlock * 4, 0.0f);
    std::memcpy(epiP.data(), epi4.data(), sizeof(float) * 4 * static_cast<size_t>(g.OC));
    int rc = plan->upload(U.data(), U.size(), &plan->d_u);
    if (rc == SNNHIP_OK) rc = plan->upload(epiP.data(), epiP.size(), &plan->d_epi);
    if (rc != SNNHIP_OK) {
        delete plan;
        return rc;
    }
    plan->inDims[0] = g.N; plan->inDims[1] = g.H; plan->inDims[2] = g.W; plan->inDims[3] = g.IC;
    plan->outDims[0] = g.N; plan->outDims[1] = g.OH; plan->outDims[2] = g.OW; plan->outDims[3] = g.OC;
    plan->flops = 2.0 * 9 * g.IC * g.OC * static_cast<double>(g.OH) * g.OW * g.N; // algorithmic (direct-convolution) count, SURVEY 8d
    plan->bytes = 4.0 * (static_cast<double>(g.N) * g.H * g.W * g.IC + static_cast<double>(g.N) * g.OH * g.OW * g.OC + static_cast<double>(g.OC) * g.IC * 9);
    const double mfmaFlops = 2.0 * 16 * 64 * 8 * ocPerBlock * static_cast<double>(plan->grid.x) * p.OCblocks * p.nChunks; // executed on the matrix pipe (padded tiles included)
    char buf[320];
    snprintf(buf, sizeof(buf), "conv2d_mfma_wino_f32_16x16x4 F(2x2,3x3) k=3x3 s=1 ic=%d oc=%d tile=%dx%dx%dpx x %doc chunk=8 lds=%zuB kgroups=%d splitK=%d mfma_flops=%.6g",
             g.IC, g.OC, TB, 2 * TTH, 2 * TTW, ocPerBlock, ldsAll, ks, p.splitK, mfmaFlops);
    plan->desc = buf;
    if (cat) { // inDims describes input 0, as the conv2d_mfma cat plan does; both inputs are read once
        plan->inDims[1] = srcH0; plan->inDims[2] = srcW0; plan->inDims[3] = g.C0;
        plan->bytes = 4.0 * (static_cast<double>(g.N) * srcH0 * srcW0 * g.C0 + static_cast<double>(g.N) * g.H * g.W * (g.IC - g.C0) + static_cast<double>(g.N) * g.OH * g.OW * g.OC +
                             static_cast<double>(g.OC) * g.IC * 9);
        plan->desc += " +concat(" + std::to_string(g.C0) + "+" + std::to_string(g.IC - g.C0) + ")";
        if (catUp) plan->desc += " +upsample(x2 on input 0)";
    }
    if (pool) { // the input, the weights and the POOLED output: the full-resolution tensor never exists (split over blockIdx.z: only as partial sums in the workspace)
        plan->outDims[1] = g.poolOH;
        plan->outDims[2] = g.poolOW;
        plan->bytes = 4.0 * (static_cast<double>(g.N) * g.H * g.W * g.IC + static_cast<double>(g.N) * g.poolOH * g.poolOW * g.OC + static_cast<double>(g.OC) * g.IC * 9);
        plan->desc += " +maxpool(2x2)";
    }
    if (plan->fusedAdd) {
        plan->desc += " +add";
        plan->bytes += 4.0 * static_cast<double>(g.N) * g.OH * g.OW * g.OC;
    }
    *out = plan;
    return SNNHIP_OK;
}

} // namespace snnhip
