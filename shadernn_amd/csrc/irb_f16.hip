// irb_f16.hip -- chain rule G on half tensors: Conv2D 1x1 (expand) -> DepthwiseConv2D 3x3 (stride 1 | 2) -> Conv2D 1x1 (project) [-> Add with the
// block input] as ONE launch on v_mfma_f32_16x16x32_f16.  fp16 NHWC in and out, fp32 accumulation, fp32 epilogues; values are rounded to half exactly
// where the three per-layer fp16 plans store a tensor: behind the expand epilogue, behind the depthwise epilogue, at the output.  With the fused Add the
// project layer's fp32 value takes the residual and the Add's activation before the one rounding of the store (conv1x1_stream's `+add`).
//
// A 256-thread block owns an 8 x 8 output tile of one image:
//   x tile    the (7 s + 3)^2 halo tile of the block input, halves [pixel][32 ceil(C / 32) + 8], staged once with 16-byte loads, zero past C and outside
//             the image; it also supplies the residual
//   slices    the hidden channels in slices of 32 = one K-step of the projection (a shorter last slice is zero-filled: zero weights and a zero epilogue
//             make its channels exact zeros through all three stages)
//   E(j)      expand: D[hidden][pixel] += We[hidden][k] X[k][pixel] for both 16-channel halves of the slice over every 16-pixel group of the halo tile,
//             groups dealt round-robin to the four waves; fp32 epilogue, ZERO outside the image (the depthwise layer pads the hidden tensor, and
//             act(BN(bias)) is not zero), rounded to half, a lane's four consecutive channels as one 8-byte store into the slice tile [pixel][32 + 8]
//   D(j)      depthwise: each wave owns 16 output pixels (two tile rows); lane (px = lane & 15, g = lane >> 4) reads its nine taps of channels
//             8 g .. 8 g + 7 (ds_read_b128), 72 fp32 FMAs against fp32 weights, fp32 epilogue, one rounding: eight halves that ARE the lane's
//   P(j)      B operand of the projection's K-step; one MFMA per 16-channel output block against the slice's project weights (16 bytes per lane
//             and block, straight from L1 / L2), accumulators in registers across all slices
//   The slice tile is double-buffered: E(j + 1) is issued in front of D(j) / P(j), one barrier per slice.
//   epilogue  scale / shift / activation in fp32 [+ x from the tile -> activation], 8-byte half stores.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "epilogue.h"
#include "irb_f16.h"
#include "snnhip_internal.h"

namespace snnhip {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct IrbF16Params {
    int N, H, W, C, Ch, Co, OH, OW, s, padx, pady;
    int KS;          // K-steps of the expand layer: ceil(C / 32)
    int NCB;         // 16-channel output blocks
    int nSlices;     // ceil(Ch / 32)
    int HWd, HP, MT; // halo tile: pixels per row (= rows), pixels, 16-pixel groups
    int xPitch;      // halves per pixel of the x tile
    int tilesX, tilesY;
    int offH, offMask; // LDS map in bytes: x tile at 0, the two hidden slice tiles, the in-image mask
    int hasRes;
    ActCfg ac1, ac2, ac3, ac4;
};

template <int KST /* compile-time bound on KS */, int NCBT /* ... on NCB */>
__global__ __launch_bounds__(256) void irb_f16_kernel(IrbF16Params p, const _Float16* __restrict__ x, const f16x8* __restrict__ weg, const float4* __restrict__ e1g,
                                                      const float4* __restrict__ dwg, const f16x8* __restrict__ wpg, const float4* __restrict__ e3g,
                                                      _Float16* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using namespace irb_f16;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), n16 = lane & 15, g = lane >> 4;
    const int mt = blockIdx.x;
    const int tx = mt % p.tilesX, ty = (mt / p.tilesX) % p.tilesY, img = mt / (p.tilesX * p.tilesY);
    const int ox0 = tx * kTile, oy0 = ty * kTile;
    const int hx0 = ox0 * p.s - p.padx, hy0 = oy0 * p.s - p.pady;
    _Float16* const xs = reinterpret_cast<_Float16*>(smem);
    _Float16* const hs = reinterpret_cast<_Float16*>(smem + p.offH);
    float* const msk = reinterpret_cast<float*>(smem + p.offMask);
    const int npx = p.MT * 16, hBuf = npx * kHPitch;

    // ---- x tile: npx pixels x 4 KS 16-byte pieces (consecutive threads = consecutive pieces of a pixel: whole pixels per wave instruction)
    {
        const int pieces = 4 * p.KS, total = npx * pieces, cp = p.C >> 3;
        const _Float16* const ximg = x + static_cast<size_t>(img) * p.H * p.W * p.C;
        for (int e = tid; e < total; e += 256) {
            const int hp = e / pieces, pc = e - hp * pieces;
            const int hy = hp / p.HWd, hx = hp - hy * p.HWd;
            const int iy = hy0 + hy, ix = hx0 + hx;
            const bool in = hp < p.HP && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (in && pc < cp) v = *reinterpret_cast<const float4*>(ximg + (static_cast<size_t>(iy) * p.W + ix) * p.C + pc * 8);
            *reinterpret_cast<float4*>(xs + hp * p.xPitch + pc * 8) = v;
            if (pc == 0) msk[hp] = in ? 1.0f : 0.0f;
        }
    }
    __syncthreads();

    // ---- E(j): the slice's 32 hidden channels over the halo tile's pixel groups wave, wave + 4, ...
    auto expand = [&](int j, _Float16* hb) {
        const f16x8* const wb = weg + static_cast<size_t>(j) * 2 * p.KS * 64;
        f16x8 a0[KST], a1[KST];
#pragma unroll
        for (int ks = 0; ks < KST; ++ks)
            if (ks < p.KS) {
                a0[ks] = wb[ks * 64 + lane];
                a1[ks] = wb[(p.KS + ks) * 64 + lane];
            }
        const float4 sc0 = e1g[j * 16 + g], sh0 = e1g[j * 16 + 4 + g], sc1 = e1g[j * 16 + 8 + g], sh1 = e1g[j * 16 + 12 + g];
        for (int t = wave; t < p.MT; t += 4) {
            const int px = t * 16 + n16;
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KST; ++ks)
                if (ks < p.KS) {
                    const f16x8 b = *reinterpret_cast<const f16x8*>(xs + px * p.xPitch + ks * kKStep + g * 8);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0[ks], b, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[ks], b, acc1, 0, 0, 0);
                }
            const bool in = msk[px] != 0.0f; // (a select, not a product: an overflowed value times zero would be a NaN)
            const float s0[4] = {sc0.x, sc0.y, sc0.z, sc0.w}, t0[4] = {sh0.x, sh0.y, sh0.z, sh0.w};
            const float s1[4] = {sc1.x, sc1.y, sc1.z, sc1.w}, t1[4] = {sh1.x, sh1.y, sh1.z, sh1.w};
            f16x4 h0, h1;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float v0 = apply_act<true>(p.ac1, fmaf(s0[i], acc0[i], t0[i]), 0.f), v1 = apply_act<true>(p.ac1, fmaf(s1[i], acc1[i], t1[i]), 0.f);
                h0[i] = static_cast<_Float16>(in ? v0 : 0.0f);
                h1[i] = static_cast<_Float16>(in ? v1 : 0.0f);
            }
            *reinterpret_cast<f16x4*>(hb + px * kHPitch + g * 4) = h0;
            *reinterpret_cast<f16x4*>(hb + px * kHPitch + 16 + g * 4) = h1;
        }
    };

    f32x4 acc[NCBT];
#pragma unroll
    for (int cb = 0; cb < NCBT; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int pl = wave * 16 + n16, oyl = pl >> 3, oxl = pl & 7; // the lane's output pixel: two tile rows per wave
    const int hp0 = oyl * p.s * p.HWd + oxl * p.s;

    // ---- D(j) + P(j)
    auto dw_project = [&](int j, const _Float16* hb) {
        const float4* const db = dwg + static_cast<size_t>(j) * (kDwSliceFloats / 4);
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int fy = 0; fy < 3; ++fy)
#pragma unroll
            for (int fx = 0; fx < 3; ++fx) {
                const f16x8 h = *reinterpret_cast<const f16x8*>(hb + (hp0 + fy * p.HWd + fx) * kHPitch + g * 8);
                const float4 w0 = db[(fy * 3 + fx) * 8 + 2 * g], w1 = db[(fy * 3 + fx) * 8 + 2 * g + 1];
                const float w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
                for (int i = 0; i < 8; ++i) s[i] = fmaf(static_cast<float>(h[i]), w[i], s[i]);
            }
        const float4 c0 = db[72 + 2 * g], c1 = db[72 + 2 * g + 1], d0 = db[80 + 2 * g], d1 = db[80 + 2 * g + 1];
        const float sc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w}, sh[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
        f16x8 b;
#pragma unroll
        for (int i = 0; i < 8; ++i) b[i] = static_cast<_Float16>(apply_act<true>(p.ac2, fmaf(sc[i], s[i], sh[i]), 0.f));
        const f16x8* const wb = wpg + static_cast<size_t>(j) * p.NCB * 64;
#pragma unroll
        for (int cb = 0; cb < NCBT; ++cb)
            if (cb < p.NCB) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb[cb * 64 + lane], b, acc[cb], 0, 0, 0);
    };

    expand(0, hs);
    __syncthreads();
    for (int j = 0; j < p.nSlices; ++j) {
        if (j + 1 < p.nSlices) expand(j + 1, hs + ((j + 1) & 1) * hBuf); // into the tile that D(j - 1) read before the last barrier
        dw_project(j, hs + (j & 1) * hBuf);
        __syncthreads();
    }

    // ---- epilogue: the lane holds output channels 16 cb + 4 g .. + 3 of its pixel
    const int oy = oy0 + oyl, ox = ox0 + oxl;
    if (oy < p.OH && ox < p.OW) {
        _Float16* const yp = y + ((static_cast<size_t>(img) * p.OH + oy) * p.OW + ox) * p.Co;
        const _Float16* const rp = xs + ((oyl + p.pady) * p.HWd + oxl + p.padx) * p.xPitch; // residual (stride 1, C == Co): the block input at the output pixel
#pragma unroll
        for (int cb = 0; cb < NCBT; ++cb) {
            const int co = cb * 16 + 4 * g;
            if (cb < p.NCB && co < p.Co) {
                const float4 sc = e3g[cb * 8 + g], sh = e3g[cb * 8 + 4 + g];
                const float s3[4] = {sc.x, sc.y, sc.z, sc.w}, t3[4] = {sh.x, sh.y, sh.z, sh.w};
                f16x4 r = {0, 0, 0, 0};
                if (p.hasRes) r = *reinterpret_cast<const f16x4*>(rp + co);
                f16x4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float v = apply_act<true>(p.ac3, fmaf(s3[i], acc[cb][i], t3[i]), 0.f);
                    if (p.hasRes) v = apply_act<true>(p.ac4, v + static_cast<float>(r[i]), 0.f); // on the fp32 value: the store is the one rounding
                    o[i] = static_cast<_Float16>(v);
                }
                *reinterpret_cast<f16x4*>(yp + co) = o;
            }
        }
    }
}

typedef void (*IrbF16Fn)(IrbF16Params, const _Float16*, const f16x8*, const float4*, const float4*, const f16x8*, const float4*, _Float16*);

// the smallest instance that holds the block: (K-steps, output blocks) of MobileNetV2's blocks
IrbF16Fn pick_irb_f16(int KS, int NCB, int* vKs, int* vNcb) {
    static const struct { int ks, ncb; IrbF16Fn fn; } kVariants[] = {{1, 2, irb_f16_kernel<1, 2>},  {1, 4, irb_f16_kernel<1, 4>},   {2, 4, irb_f16_kernel<2, 4>},  {2, 6, irb_f16_kernel<2, 6>},
                                                                    {3, 6, irb_f16_kernel<3, 6>},  {3, 10, irb_f16_kernel<3, 10>}, {5, 10, irb_f16_kernel<5, 10>}, {5, 20, irb_f16_kernel<5, 20>}};
    for (const auto& v : kVariants)
        if (KS <= v.ks && NCB <= v.ncb) {
            *vKs = v.ks;
            *vNcb = v.ncb;
            return v.fn;
        }
    return nullptr;
}

struct IrbF16Plan : snnhip_plan {
    IrbF16Params p;
    float *d_we = nullptr, *d_e1 = nullptr, *d_dw = nullptr, *d_wp = nullptr, *d_e3 = nullptr;
    size_t ldsBytes = 0;
    dim3 grid;
    IrbF16Fn kernel = nullptr;

    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        SNNHIP_REQUIRE(nIn == 1, "irb_f16: expects 1 input (the block input is also the residual), got %d", nIn);
        const snnhip_tensor* x = in[0];
        SNNHIP_REQUIRE(x->dtype == SNNHIP_F16 && out->dtype == SNNHIP_F16, "irb_f16: half tensors only (input dtype %d, output dtype %d)", x->dtype, out->dtype);
        SNNHIP_REQUIRE(x->n == p.N && x->h == p.H && x->w == p.W && x->c == p.C, "irb_f16: input dims %dx%dx%dx%d != plan %dx%dx%dx%d", x->n, x->h, x->w, x->c, p.N, p.H,
                       p.W, p.C);
        SNNHIP_REQUIRE(out->n == p.N && out->h == p.OH && out->w == p.OW && out->c == p.Co, "irb_f16: output dims %dx%dx%dx%d != plan %dx%dx%dx%d", out->n, out->h,
                       out->w, out->c, p.N, p.OH, p.OW, p.Co);
        SNNHIP_LAUNCH(kernel, grid, dim3(256), ldsBytes, ctx->stream, p, reinterpret_cast<const _Float16*>(x->data), reinterpret_cast<const f16x8*>(d_we),
                      reinterpret_cast<const float4*>(d_e1), reinterpret_cast<const float4*>(d_dw), reinterpret_cast<const f16x8*>(d_wp),
                      reinterpret_cast<const float4*>(d_e3), reinterpret_cast<_Float16*>(out->data));
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }
};

} // namespace

// The three per-layer fp16 plans (borrowed, only read) [+ the residual Add plan]; SNNHIP_E_UNSUPPORTED for whatever the kernel does not run: the
// caller keeps the per-layer plans.
int make_irb_f16_plan(snnhip_ctx* ctx, snnhip_plan* expandPlan, snnhip_plan* dwPlan, snnhip_plan* projectPlan, snnhip_plan* addPlan, snnhip_plan** out) {
    using namespace irb_f16;
    auto* ce = dynamic_cast<ConvPlanBase*>(expandPlan);
    auto* cd = dynamic_cast<ConvPlanBase*>(dwPlan);
    auto* cp = dynamic_cast<ConvPlanBase*>(projectPlan);
    auto* ad = addPlan ? dynamic_cast<EltwisePlanBase*>(addPlan) : nullptr;
    if (!ce || !cd || !cp || ce->depthwise || !cd->depthwise || cp->depthwise || (addPlan && (!ad || ad->mode != 0))) return SNNHIP_E_UNSUPPORTED;
    const ConvGeom &ge = ce->g, &gd = cd->g, &gp = cp->g;
    auto pointwise = [](const ConvGeom& g) {
        return g.kh == 1 && g.kw == 1 && g.sh == 1 && g.sw == 1 && g.preMode == 0 && g.addAct < 0 && g.dtype == SNNHIP_F16 && !g.normShift && !g.C0 && !g.poolOH;
    };
    if (!pointwise(ge) || !pointwise(gp) || gd.dtype != SNNHIP_F16 || gd.kh != 3 || gd.kw != 3 || gd.sh != gd.sw || gd.sh < 1 || gd.sh > 2 || gd.preMode != 0 || gd.normShift)
        return SNNHIP_E_UNSUPPORTED;
    if (gd.padMode != SNNHIP_PAD_CONSTANT && gd.padMode != SNNHIP_PAD_NONE) return SNNHIP_E_UNSUPPORTED; // the halo tile is zero outside the image, nothing else
    if (ge.OC != gd.IC || gd.OC != gp.IC || ge.N != gd.N || gd.N != gp.N || ge.OH != gd.H || ge.OW != gd.W || gd.OH != gp.H || gd.OW != gp.W || ge.OH != ge.H ||
        ge.OW != ge.W || gp.OH != gp.H || gp.OW != gp.W)
        return SNNHIP_E_UNSUPPORTED;
    if (gd.padx < 0 || gd.padx > 2 || gd.pady < 0 || gd.pady > 2) return SNNHIP_E_UNSUPPORTED;
    const int C = ge.IC, Ch = ge.OC, Co = gp.OC, s = gd.sh;
    // 16-byte loads of the input, eight hidden channels per lane, 8-byte stores; five K-steps of expand weights and twenty accumulator tiles per lane
    if (C % 8 || Ch % 8 || Co % 8 || C > kMaxC || Co > kMaxCo) return SNNHIP_E_UNSUPPORTED;
    const int acts[4] = {ge.act, gd.act, gp.act, ad ? ad->d.act : 0};
    for (int a : acts)
        if (!act_is_simple(a)) return SNNHIP_E_UNSUPPORTED;
    if (ad && (s != 1 || C != Co || ad->d.N != gp.N || ad->d.H != gp.OH || ad->d.W != gp.OW || ad->d.C != Co)) return SNNHIP_E_UNSUPPORTED;
    if (static_cast<double>(ge.N) * ge.H * ge.W * std::max(C, Ch) >= 2147483647.0 || static_cast<double>(gp.N) * gp.OH * gp.OW * Co >= 2147483647.0)
        return SNNHIP_E_UNSUPPORTED;
    if (ge.N < 1 || gd.OH < 1 || gd.OW < 1) return SNNHIP_E_UNSUPPORTED;
    const size_t lds = lds_bytes(C, s);
    if (lds > kMaxLds) return SNNHIP_E_UNSUPPORTED;

    IrbF16Params p = {};
    p.N = ge.N; p.H = ge.H; p.W = ge.W; p.C = C; p.Ch = Ch; p.Co = Co; p.OH = gd.OH; p.OW = gd.OW; p.s = s; p.padx = gd.padx; p.pady = gd.pady;
    p.KS = up_div(C, kKStep);
    p.NCB = up_div(Co, 16);
    p.nSlices = up_div(Ch, kSlice);
    p.HWd = halo(s);
    p.HP = p.HWd * p.HWd;
    p.MT = up_div(p.HP, 16);
    p.xPitch = x_pitch(C);
    p.tilesX = up_div(p.OW, kTile);
    p.tilesY = up_div(p.OH, kTile);
    p.offH = p.MT * 16 * p.xPitch * 2;
    p.offMask = p.offH + 2 * p.MT * 16 * kHPitch * 2;
    p.hasRes = ad ? 1 : 0;
    p.ac1 = make_act_cfg(ge.act, ge.leaky);
    p.ac2 = make_act_cfg(gd.act, gd.leaky);
    p.ac3 = make_act_cfg(gp.act, gp.leaky);
    p.ac4 = make_act_cfg(ad ? ad->d.act : 0, ad ? ad->d.leaky : 0.0f);
    if (static_cast<double>(p.tilesX) * p.tilesY * p.N >= 2147483647.0) return SNNHIP_E_UNSUPPORTED;
    int vKs = 0, vNcb = 0;
    const IrbF16Fn fn = pick_irb_f16(p.KS, p.NCB, &vKs, &vNcb);
    if (!fn) return SNNHIP_E_UNSUPPORTED;
    // dynamic LDS beyond 64 KB needs the attribute on THIS device: set at every plan creation (a process-wide 'done' flag would leave a second device
    // without it), and to the kernel's ceiling, so that it never shrinks under an earlier plan of the same instance
    if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kMaxLds)) != hipSuccess) {
        set_error("irb_f16: hipFuncSetAttribute(%zu) failed", kMaxLds);
        return SNNHIP_E_HIP;
    }

    const std::vector<_Float16> we = pack_expand(ce->w_oihw, C, Ch), wp = pack_project(cp->w_oihw, Ch, Co);
    const std::vector<float> e1 = pack_expand_epi(ce->epi4, Ch, ge.useBN), dw = pack_depthwise(cd->w_oihw, cd->epi4, Ch, gd.useBN), e3 = pack_project_epi(cp->epi4, Co, gp.useBN);
    auto* plan = new IrbF16Plan();
    plan->ctx = ctx;
    plan->p = p;
    plan->kernel = fn;
    plan->ldsBytes = lds;
    plan->grid = dim3(static_cast<unsigned>(p.tilesX * p.tilesY * p.N));
    plan->dtype = SNNHIP_F16;
    int rc = plan->upload(reinterpret_cast<const float*>(we.data()), we.size() / 2, &plan->d_we);
    if (rc == SNNHIP_OK) rc = plan->upload(e1.data(), e1.size(), &plan->d_e1);
    if (rc == SNNHIP_OK) rc = plan->upload(dw.data(), dw.size(), &plan->d_dw);
    if (rc == SNNHIP_OK) rc = plan->upload(reinterpret_cast<const float*>(wp.data()), wp.size() / 2, &plan->d_wp);
    if (rc == SNNHIP_OK) rc = plan->upload(e3.data(), e3.size(), &plan->d_e3);
    if (rc != SNNHIP_OK) {
        delete plan;
        return rc;
    }
    memcpy(plan->inDims, expandPlan->inDims, sizeof(plan->inDims));
    memcpy(plan->outDims, projectPlan->outDims, sizeof(plan->outDims));
    plan->flops = ce->flops + cd->flops + cp->flops;
    // input + output halves, half pointwise weights, fp32 depthwise weights and epilogue constants
    plan->bytes = 2.0 * (static_cast<double>(p.N) * p.H * p.W * C + static_cast<double>(p.N) * p.OH * p.OW * Co + static_cast<double>(Ch) * (C + Co)) +
                  4.0 * (static_cast<double>(Ch) * (9 + 4) + 2.0 * Co);
    plan->kernelBytes = plan->bytes;
    char buf[320];
    snprintf(buf, sizeof(buf), "irb_f16 mfma_f32_16x16x32_f16 [conv1x1 %d->%d + depthwise3x3 s%d + conv1x1 %d->%d%s] C=%d Ch=%d Co=%d stride=%d tile=8x8px per block, halo=%dx%d "
             "slices=%d lds=%zuB kernel=irb_f16_kernel<%d,%d>",
             C, Ch, s, Ch, Co, addPlan ? " + add" : "", C, Ch, Co, s, p.HWd, p.HWd, p.nSlices, lds, vKs, vNcb);
    plan->desc = buf;
    *out = plan;
    return SNNHIP_OK;
}

} // namespace snnhip
