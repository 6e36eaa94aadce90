// chain_fuse.hip -- the chain planner (make_chain_plan): a linear run of plans is rewritten into fewer launches.  No kernel lives here: every rule
// either builds a plan through a factory of the unit that owns the kernel, or a fused ESPCN launch through that unit's header (espcn_fused.h,
// espcn_d2s_mfma.h, espcn_f16.h, espcn_f16_wide.h, espcn_stream.hip's entry points in snnhip_internal.h).
//
// The reference runs one compute dispatch + one full barrier per layer (core/src/ic2/vulkanRenderpass.cpp:257-259) and round-trips every
// intermediate through a texture.  Rules, tried at every position in this order (the order is behaviour):
//   E    Conv2D (MFMA kernel) + Add                                   -> one two-input convolution plan, returned as is (never a chain)
//   C    the whole ESPCN x2 pattern, SNNHIP_ESPCN_FUSION=stream       -> one row-streaming launch (espcn_stream.hip)
//   A16 / B16   rules A / B on fp16 tensors, SNNHIP_ESPCN_F16=1       -> espcn_f16.hip
//   A16 / B16 wide   the same at the published widths 1 -> 64 -> 32 -> r*r, fp16 only, same switch   -> espcn_f16_wide.hip
//   A    conv KxK (1 -> 16) + act -> conv 3x3 (16 -> 16) + act        -> kernel A (espcn_fused.hip)
//   B    conv 3x3 (16 -> r*r) + act -> depth-to-space(r) + tanh       -> kernel B (r = 2: espcn_fused.hip; r = 3, 4: espcn_d2s_mfma.hip)
//   J, G D                                                            -> plans of conv2d_stem_f32.hip, irb_fused.hip / dwpw_march.hip, conv2d_mfma.hip
// and three passes over the steps they built: I (InstanceNorm -> convolution), F (convolution -> InstanceNorm, with H and I behind it) and the
// 8-bit ends A8 / B8 (and their fp16 forms).
#include <cstdlib>
#include <memory>

#include "espcn_d2s_mfma.h"
#include "espcn_f16.h"
#include "espcn_f16_wide.h"
#include "espcn_fused.h"
#include "snnhip_internal.h"

namespace snnhip {
namespace {

// Every switch the planner obeys, read once per plan creation (not at library load: tests flip them between plan creations).
struct Switches {
    static bool is(const char* v, const char* word) { return v && strcmp(v, word) == 0; }
    const bool noAddFusion = option("SNNHIP_NO_ADD_FUSION") != nullptr;
    // Default = the two-kernel fusion (rules A+B).  SNNHIP_ESPCN_FUSION=stream selects the single row-streaming kernel
    // (rule C, espcn_stream.hip): parity-tested, 20 B/px of HBM traffic, but measured slower on MI355X so far
    // (206 us vs 123+45 us per 1080p frame) because its per-wave dependency chain starves the matrix pipe.
    const bool stream = is(option("SNNHIP_ESPCN_FUSION"), "stream");
    const bool aDirect = is(option("SNNHIP_ESPCN_A"), "direct"); // kernel A: conv2 direct instead of Winograd F(2x2,3x3)
    const bool bWino = is(option("SNNHIP_ESPCN_B"), "wino");     // kernel B (r = 2): Winograd / 4x4x1-MFMA instead of the direct VALU kernel
    // Rules A16 / B16 (espcn_f16.hip): the same layer patterns on SNNHIP_F16 tensors, opt-in.  The fp32 alternatives (rule C, the direct kernel A,
    // the Winograd kernel B) have no fp16 form: with one of them selected the fp16 chain stays per layer.
    const char* const f16Word = option("SNNHIP_ESPCN_F16");
    const bool f16 = f16Word && f16Word[0] && strcmp(f16Word, "0") != 0 && !stream && !aDirect && !bWino;
    const bool noPadFusion = option("SNNHIP_NO_PAD_FUSION") != nullptr;
    const bool noNormFold = option("SNNHIP_NO_NORM_FOLD") != nullptr; // rule I off: the norm keeps its own normalise sweep
    const bool noWideNorm = option("SNNHIP_NO_WIDE_NORM") != nullptr;
    const char* const normFusionWord = option("SNNHIP_NORM_FUSION");
    const int normFusion = normFusionWord ? atoi(normFusionWord) : -1; // rule F: -1 default, 0 off, 1 every kernel that can
    const char* const minMbWord = option("SNNHIP_NORM_FUSION_MIN_MB");
    const double normFusionMinBytes = (minMbWord ? atof(minMbWord) : 128.0) * 1048576.0;
    const bool stemNoStats = option("SNNHIP_STEM_NO_STATS") != nullptr;
    const bool noKernelFold = option("SNNHIP_NO_KERNEL_FOLD") != nullptr;
};

bool plain_act(int act) { return act >= 0 && act <= SNNHIP_ACT_SILU; }

// (the ESPCN kernels are fp32; rules A16 / B16 -- espcn_f16.hip, SNNHIP_ESPCN_F16=1 -- ask for SNNHIP_F16)
bool is_same_conv(const ConvGeom& g, int k, int ic, int oc, int dtype = SNNHIP_F32) {
    return g.dtype == dtype && g.preMode == 0 && g.kh == k && g.kw == k && g.IC == ic && g.OC == oc && g.sh == 1 && g.sw == 1 && g.padx == k / 2 && g.pady == k / 2 &&
           (g.padMode == SNNHIP_PAD_CONSTANT || g.padMode == SNNHIP_PAD_NONE) && g.OH == g.H && g.OW == g.W && plain_act(g.act);
}
// The widths of the ESPCN pattern: C1 behind the first convolution, C2 behind the second (= what the tail reads).  The rules compare them with the
// widths their kernels are built for: (16, 16) the reference demo's reduced net, (64, 32) the published one (fp16 only, espcn_f16_wide.hip).
struct EspcnWidths {
    int c1 = 0, c2 = 0;
    bool operator==(const EspcnWidths& o) const { return c1 == o.c1 && c2 == o.c2; }
};
constexpr EspcnWidths kNarrow{16, 16}, kWide{kEspcnF16WideC1, kEspcnF16WideC2};
// the head of the ESPCN pattern (rules A, A16, A16 wide, C): conv 5x5 or 3x3 (1 -> C1) -> conv 3x3 (C1 -> C2); returns (C1, C2), or (0, 0)
EspcnWidths conv_pair_widths(const ConvPlanBase* c0, const ConvPlanBase* c1, int dtype) {
    if (!c0 || !c1 || c0->depthwise || c1->depthwise) return {};
    const EspcnWidths w{c0->g.OC, c1->g.OC};
    return ((is_same_conv(c0->g, 5, 1, w.c1, dtype) || is_same_conv(c0->g, 3, 1, w.c1, dtype)) && is_same_conv(c1->g, 3, w.c1, w.c2, dtype)) ? w : EspcnWidths{};
}
bool is_conv_pair(const ConvPlanBase* c0, const ConvPlanBase* c1, int dtype, const EspcnWidths& want = kNarrow) { return conv_pair_widths(c0, c1, dtype) == want; }
// its tail (rules B, B16, B16 wide): conv 3x3 (C2 -> r*r) -> depth-to-space(r), r = 2, 3, 4; returns r where C2 is the width asked for, or 0
int d2s_tail_factor(const ConvPlanBase* c0, const SubpixelPlanBase* sp1, int dtype, int c2 = kNarrow.c2) {
    const int r = (c0 && sp1) ? sp1->d.factor : 0;
    return (r >= 2 && r <= 4 && !c0->depthwise && is_same_conv(c0->g, 3, c2, r * r, dtype) && sp1->d.mode == SNNHIP_SUBPIXEL_D2S && sp1->d.C == r * r) ? r : 0;
}
// The fp16 tails (B16, B16 wide) behind an ESPCN head of other widths than their kernel family's -- (64, 16), (32, 32), ... -- decline: such a net
// stays per layer as a whole.  A tail with no such head in front of it (a chain that starts at the tail) is taken as before.
bool behind_other_head(const ConvPlanBase* h0, const ConvPlanBase* h1, const EspcnWidths& want) {
    const EspcnWidths head = conv_pair_widths(h0, h1, SNNHIP_F16);
    return head.c1 != 0 && !(head == want);
}
void rename_kernel(std::string& desc, const std::string& from, const std::string& to) {
    const size_t at = desc.find(from);
    if (at != std::string::npos) desc.replace(at, from.size(), to);
}

// Chain rule F: Conv2D -> InstanceNorm.  The convolution (conv2d_mfma, fp16 LDS epilogue) leaves (mean, M2) of every output tile and channel
// next to its output; the InstanceNorm's statistics sweep -- one of its three passes over the tensor -- is replaced by a fold over those
// tile records, and its normalise pass runs in place on the convolution's output.  Both plans are borrowed (the chain or the caller owns them).
struct ConvInstanceNormPlan : snnhip_plan {
    snnhip_plan* conv = nullptr; // the convolution, or the InstanceNorm -> convolution of rule I that wraps it
    snnhip_plan* norm = nullptr;
    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        int rc = conv->invoke(in, nIn, out);
        if (rc != SNNHIP_OK) return rc;
        return instancenorm_apply_tile_stats(norm, tiles, out);
    }
    TileStatsRef tiles;
};

// Graph rule I: InstanceNorm -> [UpSampling] -> [Pad] -> Conv2D.  The norm runs its statistics sweep and fold only; the convolution (a copy
// the chain owns, built with ConvGeom::normShift / normMul) reads the norm's INPUT and normalises while it stages -- the normalised tensor is never
// written or re-read.  The norm plan is borrowed: its parameters and statistics buffers are the ones the convolution was given.
struct InstanceNormConvPlan : snnhip_plan {
    snnhip_plan* norm = nullptr;
    snnhip_plan* conv = nullptr;
    TileStatsRef tiles; // rule F in front: the convolution that PRODUCED in[0] left tile statistics -- a fold over them instead of the sweep
    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        const int rc = instancenorm_run_stats(norm, in[0], &tiles);
        return rc != SNNHIP_OK ? rc : conv->invoke(in, nIn, out);
    }
};

// One fused ESPCN launch: exactly its family's parameters and device buffers (uploaded through the chain, which frees them with itself).
struct FusedLaunch {
    virtual ~FusedLaunch() = default;
    virtual int launch(snnhip_ctx* ctx, const float* x, float* y, hipEvent_t evStart, hipEvent_t evStop) const = 0;
    // true: the launch takes a dispatch-stamped event pair (snnhip_plan::profAcquire); false: the chain brackets it (profBegin / profEnd)
    virtual bool stampsItsEvents() const { return true; }
    // A frame conversion (8- or 16-bit, to / from tensors of `dtype`) next to this launch moves into it: the family keeps the frame end and renames
    // its kernel in its description.  false = this family (or the form selected) keeps the separate launch.
    virtual bool foldIn(const FrameIn&, int /*dtype*/, std::string& /*desc*/) { return false; }
    virtual bool foldOut(const FrameOut&, int /*dtype*/, std::string& /*desc*/) { return false; }
};

// A family's kernel under its three frame ends, as its description spells it (tests and launch traces know these names): the launch's own tensor
// type, an 8-bit frame, a 16-bit frame.  DESIGN.md section 4.23 has the table.
struct FrameKernels {
    std::string plain, u8, u16;
};
// What every fold checks and does: the conversion is of the launch's tensor type, the end is not folded yet, and the family's form takes frames
// (the predicate next to its launch function).
template <class Frame>
bool fold_frame(Frame& end, const Frame& f, bool sameType, bool takesFrame, const FrameKernels& k, std::string& desc) {
    if (!sameType || end.bits || !takesFrame) return false;
    end = f;
    rename_kernel(desc, "kernel=" + k.plain, "kernel=" + (f.bits == 16 ? k.u16 : k.u8));
    return true;
}

struct FusedA : FusedLaunch { // rule A and its frame forms A8 / A16-bit (SNNHIP_ESPCN_A=direct keeps the conversion's own launch)
    FusedAParams p{};
    int k1 = 5;
    bool wino = true;
    FrameIn frame;
    float *w1 = nullptr, *w2 = nullptr, *e1 = nullptr, *e2 = nullptr;
    int launch(snnhip_ctx* ctx, const float* x, float* y, hipEvent_t evStart, hipEvent_t evStop) const override {
        return espcn_fused_a_launch(ctx->stream, p, k1, wino, frame, ctx->props.multiProcessorCount, x, w1, w2, e1, e2, y, evStart, evStop);
    }
    bool foldIn(const FrameIn& f, int dtype, std::string& desc) override {
        return fold_frame(frame, f, dtype == SNNHIP_F32, espcn_fused_a_takes_frame(wino),
                          {"conv_kxk_c1o16_wino3x3_c16o16_kernel", "conv_kxk_c1o16_wino3x3_c16o16_u8_kernel", "conv_kxk_c1o16_wino3x3_c16o16_u16_kernel"}, desc);
    }
};

struct FusedB : FusedLaunch { // rule B and its frame forms: upscale 2 on espcn_fused.hip's kernel B (SNNHIP_ESPCN_B=wino keeps the conversion's own
                              // launch), 3 / 4 on the matrix-core kernel of espcn_d2s_mfma.hip
    FusedBParams p{};
    int r = 2;
    bool wino = false;
    FrameOut frame;
    float *w = nullptr, *e = nullptr;
    int launch(snnhip_ctx* ctx, const float* x, float* y, hipEvent_t evStart, hipEvent_t evStop) const override {
        if (r == 2) return espcn_fused_b_launch(ctx->stream, p, wino, frame, x, w, e, y, evStart, evStop);
        return espcn_d2s_mfma_launch(ctx->stream, r, p, frame, x, w, e, y, evStart, evStop);
    }
    bool foldOut(const FrameOut& f, int dtype, std::string& desc) override {
        if (r == 2)
            return fold_frame(frame, f, dtype == SNNHIP_F32, espcn_fused_b_takes_frame(wino),
                              {"conv3x3_c16o4_d2s_tanh_kernel", "conv3x3_c16o4_d2s_tanh_u8_kernel", "conv3x3_c16o4_d2s_tanh_u16_kernel"}, desc);
        return fold_frame(frame, f, dtype == SNNHIP_F32, espcn_d2s_mfma_takes_frame(),
                          {"conv3x3_c16oR_d2s_tanh_kernel", "conv3x3_c16oR_d2s_tanh_u8_kernel", "conv3x3_c16oR_d2s_tanh_u16_kernel"}, desc);
    }
};

// Rules A16 / B16 and their frame forms, narrow (espcn_f16.hip) or -- wide -- at the published widths (espcn_f16_wide.hip): the two units' launch
// functions have one signature and their kernel names differ by the "wide_"; the weight buffers hold halfs (espcn_f16[_wide]_pack_w1 / _w3).
struct FusedA16 : FusedLaunch {
    EspcnF16AParams p{};
    int k1 = 5;
    bool wide = false;
    FrameIn frame;
    float *w1 = nullptr, *w2 = nullptr, *e1 = nullptr, *e2 = nullptr;
    int launch(snnhip_ctx* ctx, const float* x, float* y, hipEvent_t evStart, hipEvent_t evStop) const override {
        return (wide ? espcn_f16_wide_a_launch : espcn_f16_a_launch)(ctx->stream, k1, p, frame, x, reinterpret_cast<const _Float16*>(w1),
                                                                      reinterpret_cast<const _Float16*>(w2), e1, e2, reinterpret_cast<_Float16*>(y), evStart, evStop);
    }
    bool foldIn(const FrameIn& f, int dtype, std::string& desc) override {
        const std::string k = wide ? "espcn_f16_wide_conv_pair" : "espcn_f16_conv_pair";
        return fold_frame(frame, f, dtype == SNNHIP_F16, wide ? espcn_f16_wide_takes_frame() : espcn_f16_takes_frame(),
                          {k + "_kernel", k + "_kernel<u8>", k + "_u16_kernel"}, desc);
    }
};

struct FusedB16 : FusedLaunch { // upscale 2, 3 or 4
    EspcnF16BParams p{};
    int r = 2;
    bool wide = false;
    FrameOut frame;
    float *w = nullptr, *e = nullptr;
    int launch(snnhip_ctx* ctx, const float* x, float* y, hipEvent_t evStart, hipEvent_t evStop) const override {
        return (wide ? espcn_f16_wide_b_launch : espcn_f16_b_launch)(ctx->stream, r, p, frame, reinterpret_cast<const _Float16*>(x), reinterpret_cast<const _Float16*>(w), e,
                                                                      y, evStart, evStop);
    }
    bool foldOut(const FrameOut& f, int dtype, std::string& desc) override {
        const std::string k = wide ? "espcn_f16_wide_d2s" : "espcn_f16_d2s", R = std::to_string(r);
        return fold_frame(frame, f, dtype == SNNHIP_F16, wide ? espcn_f16_wide_takes_frame() : espcn_f16_takes_frame(),
                          {k + "_kernel<" + R + ">", k + "_kernel<" + R + ",u8>", k + "_u16_kernel<" + R + ">"}, desc);
    }
};

struct FusedStream : FusedLaunch { // rule C (espcn_stream.hip): its configuration is an opaque blob; no 8-bit ends
    alignas(8) char cfg[kStreamCfgBytes] = {};
    float *w1 = nullptr, *w2 = nullptr, *w3 = nullptr, *e1 = nullptr, *e2 = nullptr, *e3 = nullptr;
    int launch(snnhip_ctx* ctx, const float* x, float* y, hipEvent_t, hipEvent_t) const override {
        return espcn_stream_launch(ctx->stream, cfg, x, w1, e1, w2, e2, w3, e3, y);
    }
    bool stampsItsEvents() const override { return false; }
};

struct Step {
    snnhip_plan* plain = nullptr;       // a plan (borrowed, or in ChainPlan::owned) ...
    std::unique_ptr<FusedLaunch> fused; // ... or one fused launch, which this step alone owns
    int outDims[4] = {0, 0, 0, 0};
    std::string desc;
    double flops = 0, bytes = 0; // algorithmic work of this launch (fused steps: inputs once + outputs once + weights)
};

struct ChainPlan : snnhip_plan {
    std::vector<Step> steps;
    std::vector<snnhip_tensor*> mids; // owned intermediates between steps
    std::vector<snnhip_plan*> owned;  // plans built by the chain itself (rule D: a convolution with the Pad layer folded into its staging)

    ~ChainPlan() override {
        for (auto* t : mids) snnhip_tensor_free(t);
        for (auto* q : owned) delete q;
    }
    int numSteps() const override { return static_cast<int>(steps.size()); }
    std::string stepDesc(int i) const override { return steps[i].desc; }
    void stepCost(int i, double* f, double* b) const override {
        *f = steps[i].flops;
        *b = steps[i].bytes;
    }
    bool profilesItself() const override { return true; }

    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        SNNHIP_REQUIRE(nIn == numInputs, "chain: expects %d input(s), got %d", numInputs, nIn);
        const snnhip_tensor* src = in[0];
        SNNHIP_REQUIRE(src->n == inDims[0] && src->h == inDims[1] && src->w == inDims[2] && src->c == inDims[3],
                       "chain: input dims %dx%dx%dx%d != plan %dx%dx%dx%d", src->n, src->h, src->w, src->c, inDims[0], inDims[1], inDims[2], inDims[3]);
        SNNHIP_REQUIRE(out->n == outDims[0] && out->h == outDims[1] && out->w == outDims[2] && out->c == outDims[3],
                       "chain: output dims %dx%dx%dx%d != plan %dx%dx%dx%d", out->n, out->h, out->w, out->c, outDims[0], outDims[1], outDims[2],
                       outDims[3]);
        for (size_t i = 0; i < steps.size(); ++i) {
            Step& s = steps[i];
            snnhip_tensor* dst = (i + 1 == steps.size()) ? out : mids[i];
            hipEvent_t evStart = nullptr, evStop = nullptr;
            TraceScope traceScope(s.desc, s.flops, s.bytes); // a plan step's plan opens its own scope inside this one
            const bool stamped = s.fused && s.fused->stampsItsEvents();
            if (profiling) {
                int rc = stamped ? profAcquire(static_cast<int>(i), &evStart, &evStop) : profBegin(static_cast<int>(i));
                if (rc != SNNHIP_OK) return rc;
            }
            // a chain with two inputs: the second one belongs to its LAST step (InstanceNorm -> Add behind a run of layers, rules F + H)
            const snnhip_tensor* two[2] = {src, nIn > 1 ? in[1] : nullptr};
            int rc = s.fused ? s.fused->launch(ctx, src->data, dst->data, evStart, evStop) : s.plain->invoke(two, (i + 1 == steps.size()) ? nIn : 1, dst);
            if (rc != SNNHIP_OK) return rc;
            if (profiling && !stamped) {
                rc = profEnd(static_cast<int>(i));
                if (rc != SNNHIP_OK) return rc;
            }
            src = dst;
        }
        return SNNHIP_OK;
    }
};

// What the rule functions share.  A rule looks at plans[i ..] and either declines (returns 0) or fills `st` and returns how many plans it consumed;
// a failure while it builds the step lands in `rc`.
struct Planner {
    snnhip_ctx* ctx;
    ChainPlan* chain;
    snnhip_plan* const* plans;
    int n;
    const Switches sw;
    int rc = SNNHIP_OK;
    int fusedCount = 0;
    template <class T>
    T* as(int i) const { return i < n ? dynamic_cast<T*>(plans[i]) : nullptr; }
    void upload(const std::vector<float>& v, float** dev) {
        if (rc == SNNHIP_OK) rc = chain->upload(v.data(), v.size(), dev);
    }
    void upload_halfs(const std::vector<_Float16>& h, float** dev) { // (plan buffers are handed out as float*: two halfs per element)
        std::vector<float> raw((h.size() + 1) / 2, 0.0f);
        memcpy(raw.data(), h.data(), h.size() * sizeof(_Float16));
        upload(raw, dev);
    }
};

// the step that stands for `used` plans: a fused launch, or a plan
int fill_step(Step& st, std::unique_ptr<FusedLaunch> f, const int* outDims, const std::string& desc, double flops, double bytes, int used) {
    st.fused = std::move(f);
    memcpy(st.outDims, outDims, sizeof(st.outDims));
    st.desc = desc;
    st.flops = flops;
    st.bytes = bytes;
    return used;
}
// ... plans[i] itself (borrowed), or -- own -- one a rule built in place of `used` plans
int wrap_plan(Planner& pl, snnhip_plan* p, bool own, int used, Step& st) {
    if (own) pl.chain->owned.push_back(p);
    st.plain = p;
    return fill_step(st, nullptr, p->outDims, p->desc, p->flops, p->bytes, used);
}

// ---- rule C: the whole ESPCN pattern as one row-streaming kernel (espcn_stream.hip)
int rule_stream(Planner& pl, int i, Step& st) {
    auto *c0 = pl.as<ConvPlanBase>(i), *c1 = pl.as<ConvPlanBase>(i + 1), *c2 = pl.as<ConvPlanBase>(i + 2);
    auto* sp3 = pl.as<SubpixelPlanBase>(i + 3);
    if (!pl.sw.stream || !is_conv_pair(c0, c1, SNNHIP_F32) || !c2 || !sp3 || c2->depthwise || !is_same_conv(c2->g, 3, 16, 4) || sp3->d.factor != 2 ||
        sp3->d.mode != SNNHIP_SUBPIXEL_D2S || sp3->d.C != 4 || memcmp(c1->outDims, c2->inDims, sizeof(int) * 4) != 0 ||
        memcmp(c2->outDims, sp3->inDims, sizeof(int) * 4) != 0)
        return 0;
    const ConvGeom& g0 = c0->g;
    const int K1 = g0.kh, taps1 = K1 * K1;
    auto f = std::make_unique<FusedStream>();
    if (espcn_stream_step_size() > sizeof(f->cfg)) {
        set_error("internal: stream cfg blob too small");
        pl.rc = SNNHIP_E_INVALID;
        return 0;
    }
    espcn_stream_configure(f->cfg, g0.N, g0.H, g0.W, K1, g0.act, g0.leaky, c1->g.act, c1->g.leaky, c2->g.act, c2->g.leaky, pl.ctx->props.multiProcessorCount);
    pl.upload(espcn_pack_conv1(c0->w_oihw.data(), K1, false), &f->w1);
    pl.upload(espcn_pack_conv3x3_lanes(c1->w_oihw.data(), 0), &f->w2);
    pl.upload(espcn_pack_stream_w3(c2->w_oihw.data()), &f->w3);
    pl.upload(fold_epilogue(c0->epi4, 16, g0.useBN), &f->e1);
    pl.upload(fold_epilogue(c1->epi4, 16, c1->g.useBN), &f->e2);
    pl.upload(fold_epilogue(c2->epi4, 4, c2->g.useBN), &f->e3);
    char buf[320];
    espcn_stream_describe(f->cfg, buf, sizeof(buf));
    const double bytes = 4.0 * (static_cast<double>(g0.N) * g0.H * g0.W * (1 + 4) + 16.0 * taps1 + 16.0 * 16 * 9 + 4.0 * 16 * 9);
    return fill_step(st, std::move(f), sp3->outDims, buf, c0->flops + c1->flops + c2->flops, bytes, 4);
}

// ---- rule A16: rule A's pattern on fp16 tensors -> kernel A16 of espcn_f16.hip
int rule_a16(Planner& pl, int i, Step& st) {
    auto *c0 = pl.as<ConvPlanBase>(i), *c1 = pl.as<ConvPlanBase>(i + 1);
    if (!pl.sw.f16 || !is_conv_pair(c0, c1, SNNHIP_F16)) return 0;
    const ConvGeom& g0 = c0->g;
    const int K1 = g0.kh, taps1 = K1 * K1;
    auto f = std::make_unique<FusedA16>();
    f->k1 = K1;
    f->p = EspcnF16AParams{g0.N, g0.H, g0.W, up_div(g0.W, kEspcnF16TW_A), up_div(g0.H, kEspcnF16TH_A), make_act_cfg(g0.act, g0.leaky),
                           make_act_cfg(c1->g.act, c1->g.leaky), 0.0f, 1.0f};
    std::vector<_Float16> w1h(kEspcnF16W1Halfs), w2h(kEspcnF16W3Halfs);
    espcn_f16_pack_w1(c0->w_oihw.data(), K1, w1h.data());
    espcn_f16_pack_w3(c1->w_oihw.data(), 0, w2h.data());
    pl.upload_halfs(w1h, &f->w1);
    pl.upload_halfs(w2h, &f->w2);
    pl.upload(fold_epilogue(c0->epi4, 16, g0.useBN), &f->e1);
    pl.upload(fold_epilogue(c1->epi4, 16, c1->g.useBN), &f->e2);
    // MFMA flops issued per tile: conv1 one 16x16x32 per 16 pixels of the halo region (the four waves take two groups a turn), conv2 four
    // 16x16x32 + one 16x16x16 per 16 pixels
    const double tilesA = static_cast<double>(f->p.tilesX) * f->p.tilesY * g0.N;
    const int groups1 = round_up(up_div((kEspcnF16TW_A + 2) * (kEspcnF16TH_A + 2), 16), 8);
    char buf[320];
    snprintf(buf, sizeof(buf), "fused[conv%dx%d(1->16)+conv3x3(16->16)] mfma_f32_16x16x32_f16 tile=%dx%d kernel=espcn_f16_conv_pair_kernel mfma_flops=%.6g",
             K1, K1, kEspcnF16TW_A, kEspcnF16TH_A, tilesA * (groups1 * 16384.0 + (kEspcnF16TW_A * kEspcnF16TH_A / 16) * (4 * 16384.0 + 8192.0)));
    const double bytes = 2.0 * (static_cast<double>(g0.N) * g0.H * g0.W * (1 + 16) + 16.0 * taps1 + 16.0 * 16 * 9);
    return fill_step(st, std::move(f), c1->outDims, buf, c0->flops + c1->flops, bytes, 2);
}

// ---- rule B16: rule B's pattern (upscale 2, 3, 4) on fp16 tensors -> kernel B16<r> of espcn_f16.hip
int rule_b16(Planner& pl, int i, Step& st) {
    auto* c0 = pl.as<ConvPlanBase>(i);
    auto* sp1 = pl.as<SubpixelPlanBase>(i + 1);
    const int r16 = pl.sw.f16 ? d2s_tail_factor(c0, sp1, SNNHIP_F16) : 0;
    if (!r16 || (i >= 2 && behind_other_head(pl.as<ConvPlanBase>(i - 2), pl.as<ConvPlanBase>(i - 1), kNarrow))) return 0;
    const ConvGeom& g0 = c0->g;
    auto f = std::make_unique<FusedB16>();
    f->r = r16;
    f->p = EspcnF16BParams{g0.N, g0.H, g0.W, up_div(g0.W, kEspcnF16TW_B), up_div(g0.H, kEspcnF16TH_B), make_act_cfg(g0.act, g0.leaky), 1.0f, 0.0f};
    std::vector<_Float16> wh(kEspcnF16W3Halfs);
    espcn_f16_pack_w3(c0->w_oihw.data(), r16, wh.data());
    pl.upload_halfs(wh, &f->w);
    pl.upload(fold_epilogue(c0->epi4, r16 * r16, g0.useBN, r16), &f->e);
    const double tilesB = static_cast<double>(f->p.tilesX) * f->p.tilesY * g0.N;
    char buf[256];
    snprintf(buf, sizeof(buf), "fused[conv3x3(16->%d)+depth_to_space(%d)+tanh] mfma_f32_16x16x32_f16 tile=%dx%d kernel=espcn_f16_d2s_kernel<%d> mfma_flops=%.6g",
             r16 * r16, r16, kEspcnF16TW_B, kEspcnF16TH_B, r16, tilesB * (kEspcnF16TW_B * kEspcnF16TH_B / 16) * (4 * 16384.0 + 8192.0));
    const double bytes = 2.0 * (static_cast<double>(g0.N) * g0.H * g0.W * (16 + r16 * r16) + static_cast<double>(r16 * r16) * 16 * 9);
    return fill_step(st, std::move(f), sp1->outDims, buf, c0->flops, bytes, 2);
}

// ---- rule A16 wide: the same pattern at the published widths (1 -> 64 -> 32) on fp16 tensors -> kernel A16 wide of espcn_f16_wide.hip
int rule_a16_wide(Planner& pl, int i, Step& st) {
    auto *c0 = pl.as<ConvPlanBase>(i), *c1 = pl.as<ConvPlanBase>(i + 1);
    if (!pl.sw.f16 || !is_conv_pair(c0, c1, SNNHIP_F16, kWide)) return 0;
    const ConvGeom& g0 = c0->g;
    constexpr int C1 = kWide.c1, C2 = kWide.c2, TW = kEspcnF16WideTW_A, TH = kEspcnF16WideTH_A;
    const int K1 = g0.kh, taps1 = K1 * K1;
    auto f = std::make_unique<FusedA16>();
    f->wide = true;
    f->k1 = K1;
    f->p = EspcnF16AParams{g0.N, g0.H, g0.W, up_div(g0.W, TW), up_div(g0.H, TH), make_act_cfg(g0.act, g0.leaky), make_act_cfg(c1->g.act, c1->g.leaky), 0.0f, 1.0f};
    std::vector<_Float16> w1h(kEspcnF16WideW1Halfs), w2h(kEspcnF16WideW2Halfs);
    espcn_f16_wide_pack_w1(c0->w_oihw.data(), C1, K1, w1h.data());
    espcn_f16_wide_pack_w3(c1->w_oihw.data(), C1, C2, 0, w2h.data());
    pl.upload_halfs(w1h, &f->w1);
    pl.upload_halfs(w2h, &f->w2);
    pl.upload(fold_epilogue(c0->epi4, C1, g0.useBN), &f->e1);
    pl.upload(fold_epilogue(c1->epi4, C2, c1->g.useBN), &f->e2);
    // MFMA flops issued per tile (16384 per 16x16x32): conv1 C1/16 per 16 pixels of the halo region (the waves take two groups a turn), conv2
    // 9 * C1/32 K-steps x C2/16 row blocks per 16 pixels
    const double tilesA = static_cast<double>(f->p.tilesX) * f->p.tilesY * g0.N;
    const int groups1 = round_up(up_div((TW + 2) * (TH + 2), 16), 2);
    char buf[320];
    snprintf(buf, sizeof(buf), "fused[conv%dx%d(1->%d)+conv3x3(%d->%d)] mfma_f32_16x16x32_f16 tile=%dx%d kernel=espcn_f16_wide_conv_pair_kernel mfma_flops=%.6g", K1, K1,
             C1, C1, C2, TW, TH, tilesA * 16384.0 * (groups1 * (C1 / 16) + (TW * TH / 16) * (9 * C1 / 32) * (C2 / 16)));
    const double bytes = 2.0 * (static_cast<double>(g0.N) * g0.H * g0.W * (1 + C2) + static_cast<double>(C1) * taps1 + static_cast<double>(C1) * C2 * 9);
    return fill_step(st, std::move(f), c1->outDims, buf, c0->flops + c1->flops, bytes, 2);
}

// ---- rule B16 wide: the tail behind it (32 -> r*r, upscale 2, 3, 4) on fp16 tensors -> kernel B16 wide<r> of espcn_f16_wide.hip
int rule_b16_wide(Planner& pl, int i, Step& st) {
    auto* c0 = pl.as<ConvPlanBase>(i);
    auto* sp1 = pl.as<SubpixelPlanBase>(i + 1);
    const int r = pl.sw.f16 ? d2s_tail_factor(c0, sp1, SNNHIP_F16, kWide.c2) : 0;
    if (!r || (i >= 2 && behind_other_head(pl.as<ConvPlanBase>(i - 2), pl.as<ConvPlanBase>(i - 1), kWide))) return 0;
    const ConvGeom& g0 = c0->g;
    constexpr int C2 = kWide.c2, TW = kEspcnF16WideTW_B, TH = kEspcnF16WideTH_B;
    auto f = std::make_unique<FusedB16>();
    f->wide = true;
    f->r = r;
    f->p = EspcnF16BParams{g0.N, g0.H, g0.W, up_div(g0.W, TW), up_div(g0.H, TH), make_act_cfg(g0.act, g0.leaky), 1.0f, 0.0f};
    std::vector<_Float16> wh(kEspcnF16WideW3Halfs);
    espcn_f16_wide_pack_w3(c0->w_oihw.data(), C2, 16, r, wh.data());
    pl.upload_halfs(wh, &f->w);
    pl.upload(fold_epilogue(c0->epi4, r * r, g0.useBN, r), &f->e);
    const double tilesB = static_cast<double>(f->p.tilesX) * f->p.tilesY * g0.N;
    char buf[256];
    snprintf(buf, sizeof(buf), "fused[conv3x3(%d->%d)+depth_to_space(%d)+tanh] mfma_f32_16x16x32_f16 tile=%dx%d kernel=espcn_f16_wide_d2s_kernel<%d> mfma_flops=%.6g", C2,
             r * r, r, TW, TH, r, tilesB * (TW * TH / 16) * (9 * C2 / 32) * 16384.0);
    const double bytes = 2.0 * (static_cast<double>(g0.N) * g0.H * g0.W * (C2 + r * r) + static_cast<double>(r * r) * C2 * 9);
    return fill_step(st, std::move(f), sp1->outDims, buf, c0->flops + sp1->flops, bytes, 2);
}

// ---- rule A: kernel A of espcn_fused.hip, conv2 as Winograd F(2x2,3x3) (default) or direct (SNNHIP_ESPCN_A=direct)
int rule_a(Planner& pl, int i, Step& st) {
    auto *c0 = pl.as<ConvPlanBase>(i), *c1 = pl.as<ConvPlanBase>(i + 1);
    if (!is_conv_pair(c0, c1, SNNHIP_F32)) return 0;
    const ConvGeom& g0 = c0->g;
    const int K1 = g0.kh, taps1 = K1 * K1, ks1 = (taps1 + 3) / 4;
    auto f = std::make_unique<FusedA>();
    f->k1 = K1;
    f->wino = !pl.sw.aDirect;
    const int aTW = f->wino ? W_TW : A_TW, aTH = f->wino ? W_TH : A_TH;
    f->p = FusedAParams{g0.N, g0.H, g0.W, up_div(g0.W, aTW), up_div(g0.H, aTH), make_act_cfg(g0.act, g0.leaky), make_act_cfg(c1->g.act, c1->g.leaky)};
    pl.upload(espcn_pack_conv1(c0->w_oihw.data(), K1, f->wino), &f->w1);
    pl.upload(f->wino ? espcn_pack_wino(c1->w_oihw.data(), 16) : espcn_pack_conv3x3_lanes(c1->w_oihw.data(), 0), &f->w2);
    pl.upload(fold_epilogue(c0->epi4, 16, g0.useBN), &f->e1);
    pl.upload(fold_epilogue(c1->epi4, 16, c1->g.useBN), &f->e2);
    // MFMA flops actually issued (2048 per v_mfma_f32_16x16x4_f32): conv1 on the halo region with K padded to a multiple
    // of 4, conv2 either direct (36 per 16 pixels) or Winograd (64 per 16 tiles = 64 pixels)
    const double tiles = static_cast<double>(f->p.tilesX) * f->p.tilesY * g0.N;
    const int c1px = (aTW + 2) * (aTH + 2);
    const double conv1 = f->wino ? 4.0 * (((((c1px + 15) / 16) + 3) / 4 + 1) / 2 * 2) * (wino_conv1_ksteps(K1) - (K1 == 5 ? 1 : 0)) : ((c1px + 15) / 16) * ks1; // (5x5: the 25th tap runs on the VALU)
    const double conv2 = f->wino ? (aTW / 2) * (aTH / 2) / 16 * 64.0 : aTW * aTH / 16 * 36.0;
    const double mfmaFlops = tiles * (conv1 + conv2) * 2048.0;
    char buf[320];
    snprintf(buf, sizeof(buf), "fused[conv%dx%d(1->16)+conv3x3(16->16)%s] mfma_f32_16x16x4 tile=%dx%d kernel=%s mfma_flops=%.6g", K1, K1,
             f->wino ? " winograd F(2x2,3x3)" : "", aTW, aTH,
             f->wino ? "conv_kxk_c1o16_wino3x3_c16o16_kernel" : "conv_kxk_c1o16_conv3x3_c16o16_kernel", mfmaFlops);
    const double bytes = 4.0 * (static_cast<double>(g0.N) * g0.H * g0.W * (1 + 16) + 16.0 * taps1 + 16.0 * 16 * 9);
    return fill_step(st, std::move(f), c1->outDims, buf, c0->flops + c1->flops, bytes, 2);
}

// ---- rule B, upscale 2: kernel B of espcn_fused.hip
int rule_b(Planner& pl, int i, Step& st) {
    auto* c0 = pl.as<ConvPlanBase>(i);
    auto* sp1 = pl.as<SubpixelPlanBase>(i + 1);
    if (d2s_tail_factor(c0, sp1, SNNHIP_F32) != 2) return 0;
    const ConvGeom& g0 = c0->g;
    auto f = std::make_unique<FusedB>();
    // default: the direct VALU kernel (35 us per 1080p frame); SNNHIP_ESPCN_B=wino selects the Winograd / 4x4x1-MFMA kernel (45 us:
    // fewer instructions, but its 80 KB tile limits residency to 2 blocks per CU and the load phases of co-resident blocks coincide).
    // Variants measured in round 1 and removed (DESIGN.md section 5 keeps the findings): persistent + LDS-DMA double buffering 56-98 us,
    // two rows per thread 36 us (same as the default: neither LDS bandwidth nor the scalar weight loads were the limiter), persistent
    // with register prefetch 50 us, persistent Winograd with a quad-granular prefetch pipeline 50 us.
    f->wino = pl.sw.bWino;
    const int bTW = f->wino ? BW_TW : B_TW, bTH = f->wino ? BW_TH : B_TH;
    f->p = espcn_b_params(g0.N, g0.H, g0.W, bTW, bTH, make_act_cfg(g0.act, g0.leaky));
    pl.upload(f->wino ? espcn_pack_wino(c0->w_oihw.data(), 4) : espcn_pack_b_direct(c0->w_oihw.data()), &f->w);
    pl.upload(fold_epilogue(c0->epi4, 4, g0.useBN), &f->e);
    char buf[200];
    snprintf(buf, sizeof(buf), "fused[conv3x3(16->4)%s+depth_to_space(2)+tanh] %s tile=%dx%d kernel=%s", f->wino ? " winograd F(2x2,3x3)" : "",
             f->wino ? "mfma_f32_4x4x1" : "valu_f32", bTW, bTH, f->wino ? "conv3x3_c16o4_wino_d2s_tanh_kernel" : "conv3x3_c16o4_d2s_tanh_kernel");
    const double bytes = 4.0 * (static_cast<double>(g0.N) * g0.H * g0.W * (16 + 4) + 4.0 * 16 * 9);
    return fill_step(st, std::move(f), sp1->outDims, buf, c0->flops, bytes, 2);
}

// ---- rule B, upscale 3 / 4: the matrix-core kernel of espcn_d2s_mfma.hip.  (SNNHIP_ESPCN_B=wino and rule C are x2-only alternatives:
// they leave this rule in force.)
int rule_b_mfma(Planner& pl, int i, Step& st) {
    auto* c0 = pl.as<ConvPlanBase>(i);
    auto* sp1 = pl.as<SubpixelPlanBase>(i + 1);
    const int rB = d2s_tail_factor(c0, sp1, SNNHIP_F32);
    if (rB != 3 && rB != 4) return 0;
    const ConvGeom& g0 = c0->g;
    auto f = std::make_unique<FusedB>();
    f->r = rB;
    f->p = espcn_b_params(g0.N, g0.H, g0.W, BR_TW, BR_TH, make_act_cfg(g0.act, g0.leaky));
    pl.upload(espcn_pack_conv3x3_lanes(c0->w_oihw.data(), rB), &f->w);
    pl.upload(fold_epilogue(c0->epi4, rB * rB, g0.useBN, rB), &f->e);
    const double tilesB = static_cast<double>(f->p.tilesX) * f->p.tilesY * g0.N;
    char buf[256];
    snprintf(buf, sizeof(buf), "fused[conv3x3(16->%d)+depth_to_space(%d)+tanh] mfma_f32_16x16x4 tile=%dx%d kernel=conv3x3_c16oR_d2s_tanh_kernel<%d> mfma_flops=%.6g",
             rB * rB, rB, BR_TW, BR_TH, rB, tilesB * (BR_TW * BR_TH / 16) * 36.0 * 2048.0);
    const double bytes = 4.0 * (static_cast<double>(g0.N) * g0.H * g0.W * (16 + rB * rB) + static_cast<double>(rB * rB) * 16 * 9);
    return fill_step(st, std::move(f), sp1->outDims, buf, c0->flops, bytes, 2);
}

// ---- rule J: Conv2D 7x7 stride 2 (RGB) -> MaxPooling2D 3x3 stride 2 (the head of ResNet-18) -> the pooling runs in the stem's epilogue
int rule_stem_pool(Planner& pl, int i, Step& st) {
    auto* c0 = pl.as<ConvPlanBase>(i);
    snnhip_plan* spool = nullptr;
    const bool built = i + 1 < pl.n && c0 && !c0->depthwise && c0->g.kh == 7 && pool2d_plan_desc(pl.plans[i + 1], nullptr) &&
                       make_conv2d_stem32_pool_plan(pl.ctx, pl.plans[i], pl.plans[i + 1], &spool) == SNNHIP_OK;
    return built ? wrap_plan(pl, spool, true, 2, st) : 0;
}

// ---- rule G with the network's stem as the 'expand' layer: Conv2D 3x3 (3 -> C channels) -> DepthwiseConv2D 3x3 -> Conv2D 1x1 (the head of
// MobileNetV2) -> the same kernel, its staging gathers the 27 image values per pixel; the stem's output never reaches memory
int rule_stem_irb(Planner& pl, int i, Step& st) {
    auto *c0 = pl.as<ConvPlanBase>(i), *c1 = pl.as<ConvPlanBase>(i + 1), *c2 = pl.as<ConvPlanBase>(i + 2);
    snnhip_plan* sirb = nullptr;
    const bool built = c0 && c1 && c2 && !c0->depthwise && c0->g.kh == 3 && c0->g.IC == 3 && c1->depthwise && !c2->depthwise &&
                       (make_stem_dwpw_march_plan(pl.ctx, pl.plans[i], pl.plans[i + 1], pl.plans[i + 2], &sirb) == SNNHIP_OK || // (large maps: the row-marching form)
                        make_irb_plan(pl.ctx, nullptr, pl.plans[i + 1], pl.plans[i + 2], nullptr, &sirb, pl.plans[i]) == SNNHIP_OK);
    return built ? wrap_plan(pl, sirb, true, 3, st) : 0;
}

// ---- rule G: Conv2D 1x1 -> DepthwiseConv2D 3x3 -> Conv2D 1x1 (an inverted-residual block without skip connection) -> one kernel
int rule_irb(Planner& pl, int i, Step& st) {
    auto *c0 = pl.as<ConvPlanBase>(i), *c1 = pl.as<ConvPlanBase>(i + 1), *c2 = pl.as<ConvPlanBase>(i + 2);
    snnhip_plan* irb = nullptr;
    const bool built = c0 && c1 && c2 && !c0->depthwise && c1->depthwise && !c2->depthwise &&
                       make_irb_plan(pl.ctx, pl.plans[i], pl.plans[i + 1], pl.plans[i + 2], nullptr, &irb) == SNNHIP_OK;
    return built ? wrap_plan(pl, irb, true, 3, st) : 0;
}

// ---- rule G without an expand layer: DepthwiseConv2D 3x3 -> Conv2D 1x1 (MobileNetV2's first block) -> the same kernel, its hidden slice is the x tile
int rule_dwpw(Planner& pl, int i, Step& st) {
    auto *c0 = pl.as<ConvPlanBase>(i), *c1 = pl.as<ConvPlanBase>(i + 1);
    snnhip_plan* dwpw = nullptr;
    const bool built = c0 && c1 && c0->depthwise && !c1->depthwise &&
                       (make_dwpw_march_plan(pl.ctx, pl.plans[i], pl.plans[i + 1], &dwpw) == SNNHIP_OK || // (large stride-1 maps: the row-marching streaming form)
                        make_irb_plan(pl.ctx, nullptr, pl.plans[i], pl.plans[i + 1], nullptr, &dwpw) == SNNHIP_OK);
    return built ? wrap_plan(pl, dwpw, true, 2, st) : 0;
}

// ---- rule D with a nearest x2 UpSampling2D in front: [UpSampling2D, Pad, Conv2D] or [UpSampling2D, Conv2D] -> one convolution launch
int rule_upsample_pad_conv(Planner& pl, int i, Step& st) {
    auto* up = pl.as<UpsamplePlanBase>(i);
    if (!up || up->d.mode != SNNHIP_UPSAMPLE_NEAREST || up->d.scale != 2.0f || up->OH != 2 * up->d.H || up->OW != 2 * up->d.W || pl.sw.noPadFusion) return 0;
    auto* pd2 = pl.as<PadPlanBase>(i + 1);
    auto* cv = pl.as<ConvPlanBase>(i + (pd2 ? 2 : 1));
    if (!cv || cv->depthwise || cv->g.preMode != 0 || cv->desc.rfind("conv2d_mfma", 0) != 0 || cv->g.N != up->d.N || cv->g.IC != up->d.C ||
        !(pd2 ? (pd2->d.H == up->OH && pd2->d.W == up->OW && cv->g.H == pd2->OH && cv->g.W == pd2->OW) : (cv->g.H == up->OH && cv->g.W == up->OW)))
        return 0;
    ConvGeom g2 = cv->g;
    g2.preMode = pd2 ? pd2->d.mode + 1 : SNNHIP_PAD_CONSTANT; // no Pad layer: an identity pad (offsets 0) in front of the upsampling
    g2.preX = pd2 ? pd2->d.padT : 0;
    g2.preY = pd2 ? pd2->d.padL : 0;
    g2.preShift = 1;
    g2.srcH = up->d.H;
    g2.srcW = up->d.W;
    snnhip_plan* fused = nullptr;
    if (make_conv2d_mfma_plan(pl.ctx, g2, cv->w_oihw.data(), cv->epi4, &fused) != SNNHIP_OK) return 0;
    return wrap_plan(pl, fused, true, pd2 ? 3 : 2, st);
}

// ---- rule D: Pad + Conv2D -> the convolution stages its tiles straight from the unpadded tensor ("reflect Pad,
// better fused into the following conv's load stage"); only the MFMA kernel has the pre-pad address path, so a convolution that was
// routed to another kernel (the channel-thin image-producing layers) keeps its separate Pad launch
int rule_pad_conv(Planner& pl, int i, Step& st) {
    auto* pd = pl.as<PadPlanBase>(i);
    auto* c1 = pl.as<ConvPlanBase>(i + 1);
    if (!pd || !c1 || c1->depthwise || c1->g.preMode != 0 || c1->g.N != pd->d.N || c1->g.H != pd->OH || c1->g.W != pd->OW || c1->g.IC != pd->d.C ||
        !(c1->desc.rfind("conv2d_mfma", 0) == 0 || c1->desc.rfind("conv2d_rowfold", 0) == 0) || pl.sw.noPadFusion)
        return 0;
    ConvGeom g2 = c1->g;
    g2.preMode = pd->d.mode + 1; // pad desc 0/1/2 = constant / replicate / reflect -> SNNHIP_PAD_CONSTANT / _REPLICATE / _REFLECT
    g2.preX = pd->d.padT;        // sic: the Pad shader shifts x by the top pad and y by the left pad (padlayerVulkan.cpp:81-82)
    g2.preY = pd->d.padL;
    g2.srcH = pd->d.H;
    g2.srcW = pd->d.W;
    snnhip_plan* fused = nullptr;
    const int frc = c1->desc.rfind("conv2d_rowfold", 0) == 0 ? make_conv2d_rowfold_plan(pl.ctx, g2, c1->w_oihw.data(), c1->epi4, &fused)
                                                              : make_conv2d_mfma_plan(pl.ctx, g2, c1->w_oihw.data(), c1->epi4, &fused);
    if (frc != SNNHIP_OK) return 0;
    fused->ctx = pl.ctx;
    return wrap_plan(pl, fused, true, 2, st);
}

int (*const kRules[])(Planner& pl, int i, Step& st) = {rule_stream, rule_a16, rule_b16, rule_a16_wide, rule_b16_wide, rule_a, rule_b, rule_b_mfma, rule_stem_pool, rule_stem_irb, rule_irb, rule_dwpw,
                           rule_upsample_pad_conv, rule_pad_conv};

// ---- rule I: an InstanceNorm step followed by a convolution step (as given, or built by rule D above) whose kernel can normalise in its
// staging (today: conv2d_mfma's fp16 kernels).  SNNHIP_NO_NORM_FOLD keeps the norm's own normalise sweep.
void pass_norm_into_conv(Planner& pl) {
    for (size_t k = 0; k + 1 < pl.chain->steps.size() && !pl.sw.noNormFold; ++k) {
        Step &a = pl.chain->steps[k], &b = pl.chain->steps[k + 1];
        if (!a.plain || !b.plain) continue;
        snnhip_instancenorm_desc nd;
        auto* cv = dynamic_cast<ConvPlanBase*>(b.plain);
        if (!cv || cv->depthwise || cv->numInputs != 1 || cv->g.normShift || !instancenorm_plan_desc(a.plain, &nd) || !act_is_simple(nd.act)) continue;
        if (nd.N != cv->inDims[0] || nd.H != cv->inDims[1] || nd.W != cv->inDims[2] || nd.C != cv->inDims[3]) continue;
        // only where the convolution already runs on a kernel that can normalise (trading conv2d_wide_f16 for the 128-pixel kernel cost more than
        // the normalise sweep saves, measured on Candy's residual blocks: 160 + 290 us apart, 600 us folded -- the wide kernel has its own form now)
        // conv2d_wide_f16 normalises in LDS behind its DMA: worth it on the 64 / 128-channel blocks (body layers 310 + 130 us apart -> 370 us), not
        // behind a fused UpSampling (the pass runs on the 4x replicated pixels) nor on the VALU-bound 32-channel blocks (64 -> 32 up-conv: 1.07 ms
        // + 0.17 ms sweep apart, 1.70 ms folded)
        const bool onWide = cv->desc.rfind("conv2d_mfma_wide_f16", 0) == 0 && !cv->g.preShift && cv->g.OC % 64 == 0;
        // conv2d_upconv (round 6) stages the LOW-RESOLUTION tensor, so its pass runs once per pixel: the 64 -> 32 up-convolution of the style graphs reads the
        // norm's input and the 944 MB normalise sweep in front of it disappears
        const bool onUpconv = cv->desc.rfind("conv2d_mfma_upconv_f16", 0) == 0 && cv->g.IC == 64;
        if (cv->desc.rfind("conv2d_mfma_f16_", 0) != 0 && cv->desc.rfind("conv2d_rowfold", 0) != 0 && !(onWide && !pl.sw.noWideNorm) && !onUpconv) continue;
        ConvGeom g2 = cv->g;
        if (!instancenorm_stat_pointers(a.plain, &g2.normShift, &g2.normMul)) continue;
        g2.normAct = nd.act;
        g2.normLeaky = nd.leaky;
        snnhip_plan* fused = nullptr;
        const int frc = cv->desc.rfind("conv2d_rowfold", 0) == 0 ? make_conv2d_rowfold_plan(pl.ctx, g2, cv->w_oihw.data(), cv->epi4, &fused)
                                                                 : make_conv2d_mfma_plan(pl.ctx, g2, cv->w_oihw.data(), cv->epi4, &fused);
        if (frc != SNNHIP_OK) continue;
        if ((onWide && fused->desc.find("conv2d_mfma_wide_f16") == std::string::npos) || (onUpconv && fused->desc.find("conv2d_mfma_upconv_f16") == std::string::npos)) { // (routed elsewhere with the norm attached: keep the separate launches)
            delete fused;
            continue;
        }
        pl.chain->owned.push_back(fused);
        auto* both = new InstanceNormConvPlan();
        both->ctx = pl.ctx;
        both->norm = a.plain;
        both->conv = fused;
        both->dtype = fused->dtype;
        both->numInputs = fused->numInputs;
        memcpy(both->inDims, fused->inDims, sizeof(both->inDims));
        memcpy(both->outDims, fused->outDims, sizeof(both->outDims));
        both->flops = a.flops + b.flops;
        both->bytes = a.bytes / 3.0 + b.bytes; // the norm's normalise sweep (one read + one write of its three passes) is gone
        both->desc = "instancenorm(statistics sweep + fold) -> " + fused->desc;
        pl.chain->owned.push_back(both);
        a.plain = both;
        a.desc = both->desc;
        a.flops = both->flops;
        a.bytes = both->bytes;
        memcpy(a.outDims, b.outDims, sizeof(a.outDims));
        pl.chain->steps.erase(pl.chain->steps.begin() + static_cast<long>(k) + 1);
        ++pl.fusedCount;
    }
}

// ---- rule F: a convolution step (as given, or one a rule above built) whose kernel can reduce its output tiles to {mean, M2} records, followed by
// a step that starts with an InstanceNorm: the norm's statistics sweep becomes a fold over those records.  The consumer is the norm itself (the
// two steps become one: conv, fold, normalise in place), the norm + Add of rule H (last step of a two-input chain), or the norm -> convolution of
// rule I.  Default: conv2d_wide_f16, conv2d_upconv and conv2d_s2march only -- their 256 / 512-pixel tiles pass through registers on their way out anyway (+3 % on the kernel, one
// tensor read saved).  SNNHIP_NORM_FUSION=1 also takes conv2d_mfma's fp16 kernel (measured a loss: its short blocks pay 45-125 us per layer
// for the statistics where the sweep costs 40), =0 switches the rule off.
void pass_conv_stats_into_norm(Planner& pl) {
    for (size_t k = 0; k + 1 < pl.chain->steps.size() && pl.sw.normFusion != 0; ++k) {
        Step &a = pl.chain->steps[k], &b = pl.chain->steps[k + 1];
        if (!a.plain || !b.plain) continue;
        auto* aIn = dynamic_cast<InstanceNormConvPlan*>(a.plain); // the producer may itself be a normalising convolution (rule I): its inner plan is the chain's
        auto* cv = dynamic_cast<ConvPlanBase*>(aIn ? aIn->conv : a.plain);
        if (!cv || cv->depthwise || cv->numInputs != 1) continue;
        if (pl.sw.normFusion < 0 && cv->desc.find("conv2d_mfma_wide_f16") == std::string::npos && cv->desc.find("conv2d_mfma_upconv_f16") == std::string::npos &&
            !(cv->desc.find("conv2d_mfma_stem_f16") != std::string::npos && !pl.sw.stemNoStats) &&
            !(cv->desc.find("row-marching") != std::string::npos && cv->desc.find(" s=2 ") != std::string::npos))
            continue;
        // small tensors (one 720p image: 17 MB per layer) are swept out of the L2 / MALL in less time than the two fold launches take
        // (Candy batch 1: 1.12 ms without the rule, 1.24 ms with it); from a few images per batch on the sweep is an HBM pass
        const double outBytes = static_cast<double>(cv->outDims[0]) * cv->outDims[1] * cv->outDims[2] * cv->outDims[3] * (cv->dtype == SNNHIP_F16 ? 2.0 : 4.0);
        if (pl.sw.normFusion < 0 && outBytes < pl.sw.normFusionMinBytes) continue;
        auto* inConv = dynamic_cast<InstanceNormConvPlan*>(b.plain);
        snnhip_plan* normPlan = inConv ? inConv->norm : b.plain;
        snnhip_instancenorm_desc nd;
        bool normAdd = false;
        if (!instancenorm_plan_desc(normPlan, &nd)) {
            normPlan = instancenorm_add_use_tile_stats(b.plain, TileStatsRef()); // probe: which norm (the reference stays empty = a sweep)
            if (!normPlan || !instancenorm_plan_desc(normPlan, &nd)) continue;
            normAdd = true;
        }
        if (nd.N != cv->outDims[0] || nd.H != cv->outDims[1] || nd.W != cv->outDims[2] || nd.C != cv->outDims[3]) continue;
        // The statistics epilogue changes the convolution plan (tile-stat buffer, LDS size, description): never switch it on in a plan the
        // caller owns -- a borrowed per-layer plan stays what it was; the chain works on its own copy (rule D's product already is chain-owned).
        bool borrowed = false;
        for (int i = 0; i < pl.n; ++i) borrowed = borrowed || pl.plans[i] == a.plain;
        if (borrowed && !aIn) {
            snnhip_plan* copy = nullptr;
            if (make_conv2d_mfma_plan(pl.ctx, cv->g, cv->w_oihw.data(), cv->epi4, &copy) != SNNHIP_OK) continue;
            auto* cc = dynamic_cast<ConvPlanBase*>(copy);
            if (!cc || !cc->enableTileStats()) {
                delete copy;
                continue;
            }
            pl.chain->owned.push_back(copy);
            cv = cc;
        } else if (!cv->enableTileStats()) {
            continue;
        }
        // the fold scratch of the norm is sized here, at plan creation: an allocation inside run() would break a hipGraph capture in progress
        if (instancenorm_reserve_tile_stats(normPlan, cv->statTilesX, cv->statTilesY) != SNNHIP_OK) continue;
        TileStatsRef tiles;
        tiles.part = cv->statPart; tiles.tilesX = cv->statTilesX; tiles.tilesY = cv->statTilesY; tiles.TH = cv->statTH; tiles.TW = cv->statTW;
        // a kernel that folds the records itself (the last block of an image: norm_fold.h) leaves nothing to launch between it and the consumer
        NormFoldTarget target;
        if (!pl.sw.noKernelFold && instancenorm_fold_target(normPlan, &target)) tiles.folded = cv->enableNormFold(target);
        if (!tiles.folded && cv->tileStatsNeedKernelFold()) { // (an allocation failed): per-block records have no fold launch -- the norm keeps its sweep
            cv->disableTileStats();
            continue;
        }
        if (aIn) {
            const size_t arrow = aIn->desc.find(" -> ");
            aIn->desc = (arrow == std::string::npos ? std::string("instancenorm") : aIn->desc.substr(0, arrow)) + " -> " + cv->desc;
            a.desc = aIn->desc;
        } else {
            a.plain = cv;
            a.desc = cv->desc;
        }
        ++pl.fusedCount;
        if (normAdd) { // rules F + H: the plan was built by the graph walk for this chain (it is the chain's to change)
            instancenorm_add_use_tile_stats(b.plain, tiles);
            b.desc = b.plain->desc;
            b.bytes *= 0.75; // the statistics sweep (one read of its four passes) is gone
            continue;
        }
        if (inConv) { // rules F + I
            inConv->tiles = tiles;
            inConv->desc = (tiles.folded ? "instancenorm(statistics from the convolution in front) -> " : "instancenorm(fold of tile stats) -> ") + inConv->conv->desc;
            b.desc = inConv->desc;
            b.bytes -= static_cast<double>(nd.N) * nd.H * nd.W * nd.C * (cv->dtype == SNNHIP_F16 ? 2.0 : 4.0);
            continue;
        }
        auto* both = new ConvInstanceNormPlan();
        both->ctx = pl.ctx;
        both->conv = aIn ? static_cast<snnhip_plan*>(aIn) : cv;
        both->norm = b.plain;
        both->tiles = tiles;
        both->dtype = cv->dtype;
        memcpy(both->inDims, cv->inDims, sizeof(both->inDims));
        memcpy(both->outDims, cv->outDims, sizeof(both->outDims));
        both->flops = a.flops + b.flops;
        both->bytes = a.bytes + b.bytes * 2.0 / 3.0;
        both->desc = a.desc + (tiles.folded ? " -> instancenorm(1 sweep) act=" : " -> instancenorm(fold of tile stats + 1 sweep) act=") + std::to_string(nd.act);
        pl.chain->owned.push_back(both);
        a.plain = both;
        a.desc = both->desc;
        a.flops = both->flops;
        a.bytes = both->bytes;
        pl.chain->steps.erase(pl.chain->steps.begin() + static_cast<long>(k) + 1);
    }
}

// ---- the frame ends (rules A8 / B8, their 16-bit and fp16 forms): a frame conversion (1 channel, of the fused launch's tensor type) next to a fused
// ESPCN launch moves into it.  u8_in / u16_in directly in front: the kernel stages the frame and normalises it; u8_out / u16_out directly behind: its
// epilogue quantises and stores the frame.  Which launches take the fold is theirs to say (FusedLaunch::foldIn / foldOut).  Both compute the
// stand-alone plans' expressions, so the fused chain's bytes are the unfused chain's.  Only at the chain's ends: a frame is never an intermediate.
struct FrameTensor { // the float side of a conversion plan
    int dtype = SNNHIP_F32;
    double pixels = 0;
    // what folding saves per pixel: the tensor element (4 or 2 bytes) becomes a frame element
    double bytes_saved(int bits) const { return ((dtype == SNNHIP_F16 ? 2 : 4) - bits / 8) * pixels; }
};
// a one-channel u16_in / u8_in plan as a FrameIn, a u16_out / u8_out plan as a FrameOut
bool frame_in_of(const snnhip_plan* plan, FrameIn* f, FrameTensor* t) {
    snnhip_u16_in_desc w;
    snnhip_u8_in_desc u;
    if (u16_in_plan_desc(plan, &w) && w.C == 1) {
        *f = FrameIn{16, w.means[0], w.norms[0], w.shift};
        *t = FrameTensor{w.dtype, static_cast<double>(w.N) * w.H * w.W};
        return true;
    }
    if (u8_in_plan_desc(plan, &u) && u.C == 1) {
        *f = FrameIn{8, u.means[0], u.norms[0], 0};
        *t = FrameTensor{u.dtype, static_cast<double>(u.N) * u.H * u.W};
        return true;
    }
    return false;
}
bool frame_out_of(const snnhip_plan* plan, FrameOut* f, FrameTensor* t) {
    snnhip_u16_out_desc w;
    snnhip_u8_out_desc u;
    if (u16_out_plan_desc(plan, &w) && w.C == 1) {
        *f = FrameOut{16, w.scale[0], w.offset[0], static_cast<float>(w.maxval), w.shift};
        *t = FrameTensor{w.dtype, static_cast<double>(w.N) * w.H * w.W};
        return true;
    }
    if (u8_out_plan_desc(plan, &u) && u.C == 1) {
        *f = FrameOut{8, u.scale[0], u.offset[0], 255.0f, 0};
        *t = FrameTensor{u.dtype, static_cast<double>(u.N) * u.H * u.W};
        return true;
    }
    return false;
}

void pass_u8_ends(Planner& pl) {
    std::vector<Step>& steps = pl.chain->steps;
    for (size_t k = 0; k + 1 < steps.size(); ++k) {
        Step &a = steps[k], &b = steps[k + 1];
        FrameIn fi;
        FrameOut fo;
        FrameTensor t;
        if (k == 0 && a.plain && b.fused && frame_in_of(a.plain, &fi, &t) && b.fused->foldIn(fi, t.dtype, b.desc)) {
            b.desc = "u" + std::to_string(fi.bits) + "_in(1ch) + " + b.desc;
            b.flops += a.flops;
            b.bytes -= t.bytes_saved(fi.bits);
            steps.erase(steps.begin() + static_cast<long>(k));
            ++pl.fusedCount;
            --k;
        } else if (k + 2 == steps.size() && a.fused && b.plain && frame_out_of(b.plain, &fo, &t) && a.fused->foldOut(fo, t.dtype, a.desc)) {
            a.desc += " + u" + std::to_string(fo.bits) + "_out(1ch)";
            a.flops += b.flops;
            a.bytes -= t.bytes_saved(fo.bits);
            memcpy(a.outDims, b.outDims, sizeof(a.outDims));
            steps.erase(steps.begin() + static_cast<long>(k) + 1);
            ++pl.fusedCount;
        }
    }
}

} // namespace

int make_chain_plan(snnhip_ctx* ctx, snnhip_plan* const* plans, int n, snnhip_plan** out) {
    const Switches sw;
    // ---- rule E: Conv2D (MFMA kernel) + Add -> one launch, the residual is added in the convolution's epilogue.  The fused plan takes TWO
    // inputs, snnhip_plan_run_n(plan, {conv input, residual}, 2, out), so it is returned as is instead of being wrapped into a ChainPlan.
    if (n == 2 && !sw.noAddFusion) {
        auto* cv = dynamic_cast<ConvPlanBase*>(plans[0]);
        auto* ad = dynamic_cast<EltwisePlanBase*>(plans[1]);
        if (cv && ad && ad->mode == 0 && !cv->depthwise && cv->g.addAct < 0 && cv->desc.rfind("conv2d_mfma", 0) == 0 && cv->g.act != SNNHIP_ACT_SILU_QUIRK &&
            ad->d.N == cv->g.N && ad->d.H == cv->g.OH && ad->d.W == cv->g.OW && ad->d.C == cv->g.OC) {
            ConvGeom g2 = cv->g;
            g2.addAct = ad->d.act;
            g2.addLeaky = ad->d.leaky;
            return make_conv2d_mfma_plan(ctx, g2, cv->w_oihw.data(), cv->epi4, out);
        }
    }
    for (int i = 0; i < n; ++i)
        if (plans[i]->numInputs != 1 && !(i == n - 1 && plans[i]->numInputs == 2)) {
            set_error("chain fusion: plan %d takes %d inputs (only the last plan of a chain may take two)", i, plans[i]->numInputs);
            return SNNHIP_E_UNSUPPORTED;
        }
    auto* chain = new ChainPlan();
    chain->ctx = ctx;
    chain->numInputs = plans[n - 1]->numInputs;
    memcpy(chain->inDims, plans[0]->inDims, sizeof(chain->inDims));
    memcpy(chain->outDims, plans[n - 1]->outDims, sizeof(chain->outDims));
    Planner pl{ctx, chain, plans, n, sw};
    for (int i = 0; i < n && pl.rc == SNNHIP_OK;) {
        // the chain must be shape-consistent
        // (a dense layer consumes any [N,H,W,C] tensor flattened in HWC order: same batch, same element count)
        auto count3 = [](const int* d) { return static_cast<long long>(d[1]) * d[2] * d[3]; };
        if (i + 1 < n && (plans[i]->outDims[0] != plans[i + 1]->inDims[0] || count3(plans[i]->outDims) != count3(plans[i + 1]->inDims))) {
            set_error("chain: plan %d output %dx%dx%dx%d does not feed plan %d input %dx%dx%dx%d", i, plans[i]->outDims[0], plans[i]->outDims[1],
                      plans[i]->outDims[2], plans[i]->outDims[3], i + 1, plans[i + 1]->inDims[0], plans[i + 1]->inDims[1], plans[i + 1]->inDims[2],
                      plans[i + 1]->inDims[3]);
            pl.rc = SNNHIP_E_INVALID;
            break;
        }
        Step st;
        int used = 0;
        for (auto rule : kRules)
            if ((used = rule(pl, i, st)) != 0 || pl.rc != SNNHIP_OK) break;
        if (pl.rc != SNNHIP_OK) break;
        if (used) ++pl.fusedCount;
        else used = wrap_plan(pl, plans[i], false, 1, st);
        chain->steps.push_back(std::move(st));
        i += used;
    }
    if (pl.rc == SNNHIP_OK) {
        pass_norm_into_conv(pl);
        pass_conv_stats_into_norm(pl);
        pass_u8_ends(pl);
    }
    int rc = pl.rc;
    if (rc == SNNHIP_OK && pl.fusedCount == 0) {
        set_error("chain fusion: no rule matches these %d plans", n);
        rc = SNNHIP_E_UNSUPPORTED;
    }
    // element type of the chain = that of its convolutions (the element-wise plans adapt to the tensors they are given)
    for (int i = 0; i < n; ++i)
        if (auto* c = dynamic_cast<ConvPlanBase*>(plans[i])) {
            chain->dtype = c->g.dtype;
            break;
        }
    for (size_t i = 0; rc == SNNHIP_OK && i + 1 < chain->steps.size(); ++i) {
        snnhip_tensor* t = nullptr;
        const int* d = chain->steps[i].outDims;
        rc = snnhip_tensor_alloc(ctx, d[0], d[1], d[2], d[3], chain->dtype, &t);
        if (rc == SNNHIP_OK) chain->mids.push_back(t);
    }
    if (rc != SNNHIP_OK) {
        delete chain;
        return rc;
    }
    for (int i = 0; i < n; ++i) {
        chain->flops += plans[i]->flops;
        chain->bytes += plans[i]->bytes;
    }
    chain->rawInput = plans[0]->anyDtype ? -1 : plans[0]->rawInput; // a chain that starts with u8_in / u16_in reads the frame, one that ends with u8_out / u16_out writes one
    chain->rawOutput = plans[n - 1]->rawOutput;
    std::string d = "chain{";
    for (size_t i = 0; i < chain->steps.size(); ++i) d += (i ? " -> " : "") + chain->steps[i].desc;
    chain->desc = d + "}";
    *out = chain;
    return SNNHIP_OK;
}

// graph walk: a plan it built for this chain (the InstanceNorm -> Add of rule H at the chain's end) becomes the chain's to delete
bool chain_adopt_plan(snnhip_plan* chain, snnhip_plan* p) {
    auto* c = dynamic_cast<ChainPlan*>(chain);
    if (!c) return false;
    c->owned.push_back(p);
    return true;
}

} // namespace snnhip
