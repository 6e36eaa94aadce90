// hipBackend.cpp -- DeviceBackend / RenderPass on top of the C-ABI (counterpart of reference core/src/ic2/vulkanBackend.cpp
// and vulkanRenderpass.cpp).  No command buffer: plans enqueue kernels on the context's HIP stream, sync() waits for it.
#include <sys/stat.h>

#include <cstdlib>

#include "../../include/snnhip.h"
#include "ic2/backend.h"
#include "ic2/genericlayer.h"
#include "snn/contextFactory.h"

using namespace snn;
using namespace snn::dp;

static void hipChk(int rc, const char* what) {
    if (rc != SNNHIP_OK) SNN_RIP("%s: %s", what, snnhip_last_error());
}

HipRenderPass::~HipRenderPass() {
    if (owns && plan) snnhip_plan_destroy(plan);
}

void HipRenderPass::run() {
    if (skip) return;
    const snnhip_tensor* in0 = rawInput ? rawInput : input->tensor();
    snnhip_tensor* out = rawOutput ? rawOutput : output->tensor();
    if (extraInputs.empty()) {
        hipChk(snnhip_plan_run(plan, in0, out), "snnhip_plan_run");
    } else {
        std::vector<const snnhip_tensor*> ins{in0};
        for (auto* t : extraInputs) ins.push_back(t->tensor());
        hipChk(snnhip_plan_run_n(plan, ins.data(), static_cast<int>(ins.size()), out), "snnhip_plan_run_n");
    }
}

bool HipRenderPass::debugPassOutput(const std::string& folder) { // vulkanBackend.cpp:132-134 naming
    if (skip) return true;
    output->saveToBIN(formatString("%s/%s pass[0].dump", folder.c_str(), name.c_str()));
    return true;
}

bool HipRenderPass::debugPassInputs(const std::string& folder) { // vulkanRenderpass.cpp:262-277 naming
    if (skip) return true;
    input->saveToBIN(formatString("%s/%s pass[0]_input.dump", folder.c_str(), name.c_str()));
    return true;
}

HipBackend::HipBackend(GpuContext* context) {
    SNN_CHK(context && context->backendType == GpuBackendType::HIP);
    ctx = static_cast<HipContext*>(context)->ctx;
}

HipBackend::~HipBackend() {
    dropRecording();
    for (auto* p : chainPlans) snnhip_plan_destroy(p);
    replacedPasses.clear();
    if (frameInPlan) snnhip_plan_destroy(frameInPlan);
    if (frameOutPlan) snnhip_plan_destroy(frameOutPlan);
    for (auto* steps : {&stepsIn, &stepsOut})
        for (auto& s : *steps) snnhip_plan_destroy(s.plan);
    for (auto* t : frameTensors) snnhip_tensor_free(t);
}

snnhip_tensor* HipBackend::ownTensor(int n, int h, int w, int c, int dtype, const char* what) {
    snnhip_tensor* t = nullptr;
    hipChk(snnhip_tensor_alloc(ctx, n, h, w, c, dtype, &t), what);
    frameTensors.push_back(t);
    return t;
}

// The upscale factor of a luma model from its two frame tensors, whose dims it returns: one channel in and out, an integer 1..4, the same on both
// axes; video frames (4:2:0: a chroma sample under every 2 x 2 luma samples) also need an even extent.
static int frameScale(const snnhip_tensor* frameIn, const snnhip_tensor* frameOut, bool needEvenExtent, int in[4], int out[4]) {
    hipChk(snnhip_tensor_dims(frameIn, in), "snnhip_tensor_dims");
    hipChk(snnhip_tensor_dims(frameOut, out), "snnhip_tensor_dims");
    const int r = out[1] / in[1];
    if (in[3] != 1 || out[3] != 1 || out[0] != in[0] || r < 1 || r > 4 || out[1] != r * in[1] || out[2] != r * in[2] || (needEvenExtent && (in[1] % 2 || in[2] % 2)))
        SNN_RIP(needEvenExtent ? "video frames need a one-channel model of even extent whose output is 1..4 times its input: %dx%dx%d -> %dx%dx%d"
                               : "colour frames need a one-channel model whose output is 1..4 times its input: %dx%dx%d -> %dx%dx%d",
                in[1], in[2], in[3], out[1], out[2], out[3]);
    return r;
}

void HipBackend::initFrames(const FrameSpec& f, int n, int inH, int inW, int inC, int outH, int outW, int outC, int dtype) {
    using Source = FrameSpec::Source;
    using Sink = FrameSpec::Sink;
    const snn_frame_io2& m = f.model;
    const float *mn = m.in_means, *nm = m.in_norms, *sc = m.out_scale, *of = m.out_offset;
    if (m.in_format & 0x100) { // SNN_IO_R16 ..: a 16-bit frame
        snnhip_u16_in_desc d{n, inH, inW, inC, dtype, {mn[0], mn[1], mn[2], mn[3]}, {nm[0], nm[1], nm[2], nm[3]}, m.in_shift};
        hipChk(snnhip_u16_in_plan_create(ctx, &d, &frameInPlan), "snnhip_u16_in_plan_create");
    } else if (m.in_format != SNN_IO_FLOAT) {
        snnhip_u8_in_desc d{n, inH, inW, inC, dtype, {mn[0], mn[1], mn[2], mn[3]}, {nm[0], nm[1], nm[2], nm[3]}};
        hipChk(snnhip_u8_in_plan_create(ctx, &d, &frameInPlan), "snnhip_u8_in_plan_create");
    }
    if (frameInPlan) frameInT = ownTensor(n, inH, inW, inC, (m.in_format & 0x100) ? SNNHIP_U16 : SNNHIP_U8, "snnhip_tensor_alloc (input frame)");
    if (m.out_format & 0x100) {
        snnhip_u16_out_desc d{n, outH, outW, outC, dtype, {sc[0], sc[1], sc[2], sc[3]}, {of[0], of[1], of[2], of[3]}, m.out_maxval, m.out_shift};
        hipChk(snnhip_u16_out_plan_create(ctx, &d, &frameOutPlan), "snnhip_u16_out_plan_create");
    } else if (m.out_format != SNN_IO_FLOAT) {
        snnhip_u8_out_desc d{n, outH, outW, outC, dtype, {sc[0], sc[1], sc[2], sc[3]}, {of[0], of[1], of[2], of[3]}};
        hipChk(snnhip_u8_out_plan_create(ctx, &d, &frameOutPlan), "snnhip_u8_out_plan_create");
    }
    if (frameOutPlan) frameOutT = ownTensor(n, outH, outW, outC, (m.out_format & 0x100) ? SNNHIP_U16 : SNNHIP_U8, "snnhip_tensor_alloc (output frame)");
    uploadT = frameInT;
    downloadT = frameOutT;
    if (f.source == Source::MODEL && f.sink == Sink::MODEL) return;
    if (f.source == Source::YUV420_TENSOR) { // a 4:2:0 frame of any even size straight into the model's own (float) input tensor: one launch in front
        const int sd = f.wide ? SNNHIP_U16 : SNNHIP_U8;
        planarChroma = planarChromaOut = f.planar;
        uploadT = ownTensor(n, f.srcH, f.srcW, 1, sd, "snnhip_tensor_alloc (luma input plane)");
        chromaInT = ownTensor(f.planar ? 2 * n : n, f.srcH / 2, f.srcW / 2, f.planar ? 1 : 2, sd, "snnhip_tensor_alloc (chroma input plane)");
        snnhip_yuv_tensor_desc d{n, f.srcH, f.srcW, inH, inW, inC, sd, dtype, f.maxval, f.shift, f.siting, f.range, f.kr, f.kb, f.filter,
                                 {f.tensorMeans[0], f.tensorMeans[1], f.tensorMeans[2]}, {f.tensorNorms[0], f.tensorNorms[1], f.tensorNorms[2]}, f.alpha};
        snnhip_plan* p = nullptr;
        if (f.planar) hipChk(snnhip_yuv_tensor_planar_plan_create(ctx, &d, &p), "snnhip_yuv_tensor_planar_plan_create");
        else hipChk(snnhip_yuv_tensor_plan_create(ctx, &d, &p), "snnhip_yuv_tensor_plan_create");
        stepsIn.push_back({p, uploadT, chromaInT, nullptr, "[yuv tensor]", "snnhip_plan_run_n (video frame -> input tensor)"}); // out: the model's input tensor, bound at run
    }
    if (f.sink == Sink::YUV420_FROM_TENSOR) { // the model's own (float) output tensor straight to the planes of a 4:2:0 frame of its extent: one launch behind
        const int ed = f.encWide ? SNNHIP_U16 : SNNHIP_U8;
        planarChromaOut = f.encPlanar;
        lumaChromaFromTensor = true;
        downloadT = ownTensor(n, outH, outW, 1, ed, "snnhip_tensor_alloc (luma output plane)");
        chromaOutT = ownTensor(f.encPlanar ? 2 * n : n, outH / 2, outW / 2, f.encPlanar ? 1 : 2, ed, "snnhip_tensor_alloc (chroma output plane)");
        snnhip_tensor_yuv_desc d{n, outH, outW, outC, dtype, ed, f.encMaxval, f.encShift, f.encSiting, f.encRange, f.encKr, f.encKb,
                                 {f.encScale[0], f.encScale[1], f.encScale[2]}, {f.encOffset[0], f.encOffset[1], f.encOffset[2]}};
        snnhip_plan* p = nullptr;
        if (f.encPlanar) hipChk(snnhip_tensor_yuv_planar_plan_create(ctx, &d, &p), "snnhip_tensor_yuv_planar_plan_create");
        else hipChk(snnhip_tensor_yuv_plan_create(ctx, &d, &p), "snnhip_tensor_yuv_plan_create");
        stepsOut.push_back({p, nullptr, nullptr, downloadT, "[tensor yuv]", "snnhip_plan_run_io (output tensor -> video frame)", chromaOutT}); // in: the model's output tensor, bound at run
    }
    if (f.source == Source::YUV420_TENSOR || f.sink == Sink::YUV420_FROM_TENSOR) return;

    // colour or video frames around a luma-only model: the luma plane IS the model's frame at a video end
    const int vd = f.wide ? SNNHIP_U16 : SNNHIP_U8;
    SNN_CHK(frameInT && frameOutT && snnhip_tensor_dtype(frameInT) == vd && snnhip_tensor_dtype(frameOutT) == vd);
    int in[4], out[4];
    const int r = frameScale(frameInT, frameOutT, f.source == Source::YUV420, in, out);
    const int cc = f.planar ? 1 : 2, cn = f.planar ? 2 * in[0] : in[0]; // planar: every Cb and Cr plane is an image of one channel
    planarChroma = planarChromaOut = f.planar;
    snnhip_plan* p = nullptr;
    if (f.source == Source::RGB) { // the colour frame's luma plane into the model's input frame
        snnhip_rgb_luma_desc d{in[0], in[1], in[2], f.channels, f.kr, f.kb};
        hipChk(snnhip_rgb_luma_plan_create(ctx, &d, &p), "snnhip_rgb_luma_plan_create");
        uploadT = ownTensor(in[0], in[1], in[2], f.channels, SNNHIP_U8, "snnhip_tensor_alloc (colour input frame)");
        stepsIn.push_back({p, uploadT, nullptr, frameInT, "[colour in]", "snnhip_plan_run (colour frame -> luma)"});
    } else {
        chromaInT = ownTensor(cn, in[1] / 2, in[2] / 2, cc, vd, "snnhip_tensor_alloc (chroma input plane)");
    }
    switch (f.sink) {
    case Sink::MODEL: break;
    case Sink::RGB_MERGED: { // the model's output frame merged with the colour frame's upsampled chroma
        snnhip_ycc_merge_desc d{in[0], in[1], in[2], f.channels, r, f.kr, f.kb};
        hipChk(snnhip_ycc_merge_plan_create(ctx, &d, &p), "snnhip_ycc_merge_plan_create");
        downloadT = ownTensor(out[0], out[1], out[2], f.channels, SNNHIP_U8, "snnhip_tensor_alloc (colour output frame)");
        stepsOut.push_back({p, frameOutT, uploadT, downloadT, "[colour out]", "snnhip_plan_run_n (luma + chroma -> colour frame)"});
        break;
    }
    case Sink::CHROMA_UP: { // the chroma planes r-fold
        snnhip_chroma_up_desc d{cn, in[1] / 2, in[2] / 2, cc, r, vd, f.maxval, f.shift, f.siting};
        hipChk(snnhip_chroma_up_plan_create(ctx, &d, &p), "snnhip_chroma_up_plan_create");
        chromaOutT = ownTensor(cn, out[1] / 2, out[2] / 2, cc, vd, "snnhip_tensor_alloc (chroma output plane)");
        stepsOut.push_back({p, chromaInT, nullptr, chromaOutT, "[chroma out]", "snnhip_plan_run (chroma plane)"});
        break;
    }
    case Sink::FITTED: { // the model's output luma frame and the ORIGINAL chroma planes, each resampled to the target (no r-fold chroma)
        snnhip_plane_fit_desc ld{out[0], out[1], out[2], 1, f.fitH, f.fitW, vd, f.maxval, f.shift, SNNHIP_SITING_CENTRE}; // a luma plane always uses centre
        hipChk(snnhip_plane_fit_plan_create(ctx, &ld, &p), "snnhip_plane_fit_plan_create (luma)");
        downloadT = ownTensor(out[0], f.fitH, f.fitW, 1, vd, "snnhip_tensor_alloc (fitted luma plane)");
        stepsOut.push_back({p, frameOutT, nullptr, downloadT, "[luma fit]", "snnhip_plan_run (luma frame -> fitted luma plane)"});
        snnhip_plane_fit_desc cd{cn, in[1] / 2, in[2] / 2, cc, f.fitH / 2, f.fitW / 2, vd, f.maxval, f.shift, f.siting};
        hipChk(snnhip_plane_fit_plan_create(ctx, &cd, &p), "snnhip_plane_fit_plan_create (chroma)");
        chromaOutT = ownTensor(cn, f.fitH / 2, f.fitW / 2, cc, vd, "snnhip_tensor_alloc (fitted chroma plane)");
        stepsOut.push_back({p, chromaInT, nullptr, chromaOutT, "[chroma fit]", "snnhip_plan_run (chroma plane -> fitted chroma plane)"});
        break;
    }
    case Sink::RGB_FROM_YUV: { // the model's output luma frame and the ORIGINAL chroma planes to packed RGB (no r-fold chroma)
        snnhip_yuv_rgb_desc d{in[0], in[1] / 2, in[2] / 2, f.channels, r, vd, f.maxval, f.shift, f.siting, f.range, f.kr, f.kb};
        if (f.planar) hipChk(snnhip_yuv_rgb_planar_plan_create(ctx, &d, &p), "snnhip_yuv_rgb_planar_plan_create");
        else hipChk(snnhip_yuv_rgb_plan_create(ctx, &d, &p), "snnhip_yuv_rgb_plan_create");
        downloadT = ownTensor(out[0], out[1], out[2], f.channels, vd, "snnhip_tensor_alloc (RGB output frame)");
        stepsOut.push_back({p, frameOutT, chromaInT, downloadT, "[rgb out]", "snnhip_plan_run_n (luma + chroma plane -> RGB frame)"});
        break;
    }
    case Sink::RGB_FROM_YUV_FITTED:
    case Sink::RGB_MERGED_FITTED: { // the model's output luma frame resampled to the target, then RGB from it and the ORIGINAL chroma source (no r-fold chroma or RGB frame)
        const bool video = f.sink == Sink::RGB_FROM_YUV_FITTED;
        snnhip_plane_fit_desc ld{out[0], out[1], out[2], 1, f.fitH, f.fitW, vd, video ? f.maxval : 255, video ? f.shift : 0, SNNHIP_SITING_CENTRE}; // as Sink::FITTED
        hipChk(snnhip_plane_fit_plan_create(ctx, &ld, &p), "snnhip_plane_fit_plan_create (luma)");
        snnhip_tensor* lumaFitT = ownTensor(out[0], f.fitH, f.fitW, 1, vd, "snnhip_tensor_alloc (fitted luma plane)");
        stepsOut.push_back({p, frameOutT, nullptr, lumaFitT, "[luma fit]", "snnhip_plan_run (luma frame -> fitted luma plane)"});
        const int source = !video ? SNNHIP_RGB_FIT_RGB : f.planar ? SNNHIP_RGB_FIT_PLANAR : SNNHIP_RGB_FIT_CBCR;
        snnhip_rgb_fit_desc d{in[0], video ? in[1] / 2 : in[1], video ? in[2] / 2 : in[2], f.fitH, f.fitW, f.channels, source, vd, f.maxval, f.shift, f.siting, f.range, f.kr, f.kb};
        hipChk(snnhip_rgb_fit_plan_create(ctx, &d, &p), "snnhip_rgb_fit_plan_create");
        downloadT = ownTensor(out[0], f.fitH, f.fitW, f.channels, vd, "snnhip_tensor_alloc (fitted RGB output frame)");
        stepsOut.push_back({p, lumaFitT, video ? chromaInT : uploadT, downloadT, "[rgb fit]", "snnhip_plan_run_n (fitted luma plane + chroma source -> RGB frame)"});
        break;
    }
    case Sink::YUV420_FROM_RGB: { // the model's output frame IS the luma plane; the chroma planes from the colour input frame
        if (r < 2 || out[1] % 2 || out[2] % 2) SNN_RIP("an NV12 output frame needs r = 2..4 and an even extent: %dx%d -> %dx%d", in[1], in[2], out[1], out[2]);
        snnhip_rgb_cbcr_desc d{in[0], in[1], in[2], f.channels, r, f.siting, f.range, f.kr, f.kb};
        if (f.planar) hipChk(snnhip_rgb_cbcr_planar_plan_create(ctx, &d, &p), "snnhip_rgb_cbcr_planar_plan_create");
        else hipChk(snnhip_rgb_cbcr_plan_create(ctx, &d, &p), "snnhip_rgb_cbcr_plan_create");
        chromaOutT = ownTensor(f.planar ? 2 * out[0] : out[0], out[1] / 2, out[2] / 2, cc, SNNHIP_U8, "snnhip_tensor_alloc (chroma output plane)");
        stepsOut.push_back({p, uploadT, nullptr, chromaOutT, "[chroma out]", "snnhip_plan_run (colour frame -> chroma plane)"});
        lumaChromaFromRgb = true;
        break;
    }
    }
}

std::string HipBackend::describeFrames() const {
    std::string s;
    char buf[320];
    for (auto* steps : {&stepsIn, &stepsOut})
        for (auto& st : *steps)
            if (snnhip_plan_describe(st.plan, buf, sizeof(buf)) == SNNHIP_OK) s += std::string(st.label) + " " + buf + "\n";
    return s;
}

void HipBackend::runSteps(const std::vector<FrameStep>& steps, snnhip_tensor* modelInput, const snnhip_tensor* modelOutput) {
    for (auto& s : steps) {
        const snnhip_tensor* ins[2] = {s.in0 ? s.in0 : modelOutput, s.in1}; // (a step without an input of its own reads the model's output tensor)
        snnhip_tensor* out = s.out ? s.out : modelInput; // (a step without a tensor of its own writes the model's input tensor)
        if (s.out1) { // two outputs
            snnhip_tensor* outs[2] = {out, s.out1};
            hipChk(snnhip_plan_run_io(s.plan, ins, s.in1 ? 2 : 1, outs, 2), s.what);
        } else {
            hipChk(s.in1 ? snnhip_plan_run_n(s.plan, ins, 2, out) : snnhip_plan_run(s.plan, ins[0], out), s.what);
        }
    }
}

void HipBackend::runFrameIn(const ImageTexture& modelInput) {
    runSteps(stepsIn, modelInput.tensor());
    if (frameInPlan && !frameInFused) hipChk(snnhip_plan_run(frameInPlan, frameInT, modelInput.tensor()), "snnhip_plan_run (frame in)");
}

void HipBackend::runFrameOut(const ImageTexture& lastOutput) {
    if (frameOutPlan && !frameOutFused) hipChk(snnhip_plan_run(frameOutPlan, lastOutput.tensor(), frameOutT), "snnhip_plan_run (frame out)");
    runSteps(stepsOut, nullptr, lastOutput.tensor());
}

// counterpart of VulkanBackend::initRenderPasses -> VulkanRenderPass ctor (vulkanBackend.cpp:43-78, vulkanRenderpass.cpp:103-178):
// this is where weights go to the device.
void HipBackend::initRenderPasses(GenericModelLayer* layer, ImageTextureArrayAccessor in, ImageTextureArrayAccessor out) {
    const InferencePasses* passes = layer->getPasses();
    SNN_CHK(passes && !passes->passes.empty());
    SNN_CHK(in.size() >= 1 && out.size() >= 1);
    auto& rps = layer->getRenderPasses();
    rps.clear();
    for (const auto& pass : passes->passes) {
        snnhip_plan* plan = nullptr;
        hipChk(pass.createPlan(ctx, &plan), pass.source.c_str());
        int od[4];
        hipChk(snnhip_plan_output_dims(plan, od), "snnhip_plan_output_dims");
        ImageTexture& o = out[0];
        // Dense produces [1][1][1][Out] while the reference's texture is Out x 1 x 1: accept both, reject real mismatches
        const size_t want = static_cast<size_t>(od[0]) * od[1] * od[2] * od[3];
        const size_t have = static_cast<size_t>(o.batch()) * o.width() * o.height() * o.channels();
        if (want != have) SNN_RIP("%s: plan output %dx%dx%dx%d does not match texture %s", layer->getName().c_str(), od[0], od[1], od[2], od[3], o.getTextureInfo2().c_str());
        auto rp = std::make_shared<HipRenderPass>(plan, &in[0], &o, layer->getName(), true);
        for (size_t k = 1; k < in.size(); ++k) rp->extraInputs.push_back(&in[k]);
        rps.push_back(rp);
        char buf[256];
        snnhip_plan_describe(plan, buf, sizeof(buf));
        SNN_LOGD("%s -> %s", layer->getName().c_str(), buf);
    }
}

bool HipBackend::sync() {
    hipChk(snnhip_sync(ctx), "snnhip_sync");
    return true;
}

bool HipBackend::beginRecord() {
    dropRecording();
    return snnhip_graph_begin_capture(ctx) == SNNHIP_OK;
}

bool HipBackend::endRecord() {
    snnhip_graph* g = nullptr;
    if (snnhip_graph_end_capture(ctx, &g) != SNNHIP_OK) return false;
    recording = g;
    return true;
}

bool HipBackend::replay() { return recording && snnhip_graph_launch(static_cast<snnhip_graph*>(recording)) == SNNHIP_OK; }

void HipBackend::dropRecording() {
    if (recording) snnhip_graph_destroy(static_cast<snnhip_graph*>(recording));
    recording = nullptr;
}

bool HipBackend::forkSide() { return snnhip_ctx_fork(ctx) == SNNHIP_OK; }
void HipBackend::backToMain() { hipChk(snnhip_ctx_main(ctx), "snnhip_ctx_main"); }
void HipBackend::joinSide() { hipChk(snnhip_ctx_join(ctx), "snnhip_ctx_join"); }
bool HipBackend::groupBegin() { return snnhip_ctx_group_begin(ctx) == SNNHIP_OK; }
void HipBackend::groupEnd() { hipChk(snnhip_ctx_group_end(ctx), "snnhip_ctx_group_end"); }

DeviceTimer* HipBackend::createDeviceTimer(const std::string& name) { return new HipDeviceTimer(ctx, name); }

void HipBackend::postRun(RenderStagesArray&, bool dumpOutput, const std::string& folder) {
    (void) folder;
    (void) dumpOutput; // dumps are written by the layers' render passes right after they run (GenericModelLayer::run)
}

// Hand the stage DAG to snnhip_graph_fuse (the library's single fusion pass: residual Conv2D -> Add pairs and linear runs, rules A-F of
// snnhip_chain_plan_create) and install the fused plans it returns.  A fused plan sits at the LAST stage of its group and reads the
// group's external inputs; the other stages of the group keep their textures un-produced and their passes skipped.
void HipBackend::finalizeStages(RenderStagesArray& stages, bool dumpOutputs, bool fuseChains) {
    if (dumpOutputs || !fuseChains) return; // dumps need every intermediate tensor
    auto passOf = [&](size_t i) -> HipRenderPass* {
        auto* ml = static_cast<GenericModelLayer*>(stages[i].layer->modelLayer);
        if (!ml || stages[i].layer->isInputLayer || stages[i].backend != Backend::Backend_GPU || ml->getRenderPasses().size() != 1) return nullptr;
        return dynamic_cast<HipRenderPass*>(ml->getRenderPasses()[0].get());
    };
    // node space: [u8_in frame conversion] + one node per stage + [u8_out frame conversion]; the conversions are ordinary plan nodes, so the
    // chain rules see them (rules A8 / B8 fold them into the ESPCN kernels)
    const int S = static_cast<int>(stages.size());
    // the input layer's stage stands for model input 0 (its texture is the bound input): with an 8-bit input its node carries the u8_in plan, so the
    // conversion sits right in front of its consumer in the linear run (a model without an input-layer stage gets an extra node 0 instead)
    int inStage = -1;
    for (size_t i = 0; i < stages.size() && inStage < 0; ++i)
        if (stages[i].layer->isInputLayer && stages[i].layer->inputIndex == 0) inStage = static_cast<int>(i);
    const int off = (frameInPlan && inStage < 0) ? 1 : 0;
    const int inNode = frameInPlan ? (off ? 0 : inStage) : -1;
    const int n = S + off + (frameOutPlan ? 1 : 0);
    std::vector<snnhip_graph_node> gnodes(static_cast<size_t>(n));
    std::vector<snnhip_fused_node> gfused(static_cast<size_t>(n));
    auto setFrameInNode = [&]() {
        if (inNode < 0) return;
        gnodes[static_cast<size_t>(inNode)] = snnhip_graph_node{};
        gnodes[static_cast<size_t>(inNode)].plan = frameInPlan;
        gnodes[static_cast<size_t>(inNode)].n_inputs = 1;
        gnodes[static_cast<size_t>(inNode)].inputs[0] = -1;
    };
    for (size_t i = 0; i < stages.size(); ++i) {
        snnhip_graph_node& nd = gnodes[i + static_cast<size_t>(off)];
        nd = snnhip_graph_node{};
        HipRenderPass* rp = passOf(i);
        nd.plan = rp ? rp->plan : nullptr;
        nd.keep = (i + 1 == stages.size() && !frameOutPlan) ? 1 : 0; // the model output (the reference binds the last stage's texture, core.cpp:219-227)
        if (stages[i].inputIds.size() > SNNHIP_GRAPH_MAX_INPUTS) nd.plan = nullptr;
        nd.n_inputs = nd.plan ? static_cast<int>(stages[i].inputIds.size()) : 0;
        for (int k = 0; k < nd.n_inputs; ++k) {
            const bool modelInput = stages[i].delayBindMask[static_cast<size_t>(k)] != 0;
            const int id = stages[i].inputIds[static_cast<size_t>(k)];
            nd.inputs[k] = modelInput ? ((inNode >= 0 && id == 0) ? inNode : -(id + 1)) : id + off;
        }
    }
    setFrameInNode();
    if (frameOutPlan) {
        snnhip_graph_node& nd = gnodes[static_cast<size_t>(n - 1)];
        nd = snnhip_graph_node{};
        nd.plan = frameOutPlan;
        nd.n_inputs = 1;
        nd.inputs[0] = S - 1 + off;
        nd.keep = 1;
    }
    // an opaque stage (CPU layer, multi-pass layer) still consumes its producers: they must stay materialised
    for (size_t i = 0; i < stages.size(); ++i)
        if (!gnodes[i + static_cast<size_t>(off)].plan)
            for (size_t k = 0; k < stages[i].inputIds.size(); ++k) {
                if (!stages[i].delayBindMask[k] && stages[i].inputIds[k] >= 0) gnodes[static_cast<size_t>(stages[i].inputIds[k] + off)].keep = 1;
                if (inNode >= 0 && stages[i].delayBindMask[k] && stages[i].inputIds[k] == 0 && static_cast<int>(i) != inStage)
                    gnodes[static_cast<size_t>(inNode)].keep = 1;
            }
    if (frameOutPlan && !gnodes[static_cast<size_t>(S - 1 + off)].plan) gnodes[static_cast<size_t>(S - 1 + off)].keep = 1;
    hipChk(snnhip_graph_fuse(ctx, gnodes.data(), n, gfused.data()), "snnhip_graph_fuse");
    frameInFused = inNode >= 0 && !gfused[static_cast<size_t>(inNode)].plan;
    frameOutFused = frameOutPlan && gfused[static_cast<size_t>(n - 1)].owned;
    // back to stage space: node 0 (the unfolded u8_in) is model input 0 again (it writes the model's input texture); a u8_out folded into a fused plan
    // moves that plan onto the last stage, which then writes the output frame
    auto toStage = [&](int id) { return id < 0 ? id : (off && id == 0) ? -1 : id - off; };
    std::vector<snnhip_graph_node> nodes(stages.size());
    std::vector<snnhip_fused_node> fused(stages.size());
    for (size_t i = 0; i < stages.size(); ++i) {
        nodes[i] = gnodes[i + static_cast<size_t>(off)];
        fused[i] = gfused[i + static_cast<size_t>(off)];
        if (frameOutFused && static_cast<int>(i) == S - 1) fused[i] = gfused[static_cast<size_t>(n - 1)];
        for (int k = 0; k < nodes[i].n_inputs; ++k) nodes[i].inputs[k] = toStage(nodes[i].inputs[k]);
        for (int k = 0; k < fused[i].n_inputs; ++k) fused[i].inputs[k] = toStage(fused[i].inputs[k]);
    }
    if (inStage >= 0 && !off && frameInPlan) { // the input layer's stage launches nothing itself: the u8_in node was only borrowed
        nodes[static_cast<size_t>(inStage)] = snnhip_graph_node{};
        fused[static_cast<size_t>(inStage)] = snnhip_fused_node{};
    }
    // which texture carries input `id` of a fused plan: the stage output, or (model inputs, bound at run()) the input slot of the stage that named it
    auto textureOf = [&](size_t groupLast, int id) -> ImageTexture* {
        if (id >= 0) return &stages[static_cast<size_t>(id)].stageOutputs[0];
        for (size_t s = 0; s <= groupLast; ++s)
            for (size_t k = 0; k < stages[s].inputIds.size(); ++k)
                if (stages[s].delayBindMask[k] && -(stages[s].inputIds[k] + 1) == id) return &stages[s].stageInputs[k];
        SNN_RIP("finalizeStages: model input %d is not bound by any stage", -id - 1);
        return nullptr;
    };
    for (size_t i = 0; i < stages.size(); ++i) {
        if (!nodes[i].plan) continue;
        HipRenderPass* rp = passOf(i);
        if (!fused[i].plan) { // folded into a later stage's plan
            rp->skip = true;
            stages[i].fusedAway = true;
            continue;
        }
        bool rewired = fused[i].n_inputs != nodes[i].n_inputs;
        for (int k = 0; k < fused[i].n_inputs && !rewired; ++k) rewired = fused[i].inputs[k] != nodes[i].inputs[k];
        if (!fused[i].owned && !rewired) continue;
        if (fused[i].owned) chainPlans.push_back(fused[i].plan); // a re-wired own plan stays owned by the pass kept in replacedPasses
        auto* ml = static_cast<GenericModelLayer*>(stages[i].layer->modelLayer);
        replacedPasses.push_back(ml->getRenderPasses()[0]); // its plan may still be launched by the fused one (unfused steps of a chain)
        auto np = std::make_shared<HipRenderPass>(fused[i].plan, textureOf(i, fused[i].inputs[0]), rp->output, rp->name + " (+fused)", false);
        for (int k = 1; k < fused[i].n_inputs; ++k) np->extraInputs.push_back(textureOf(i, fused[i].inputs[k]));
        if (frameInFused && gfused[static_cast<size_t>(frameOutFused && static_cast<int>(i) == S - 1 ? n - 1 : static_cast<int>(i) + off)].inputs[0] == -1)
            np->rawInput = frameInT; // (in node space, -1 = the u8_in node's own input: the 8-bit frame)
        if (frameOutFused && static_cast<int>(i) == S - 1) np->rawOutput = frameOutT;
        ml->getRenderPasses()[0] = np;
        char buf[512];
        snnhip_plan_describe(fused[i].plan, buf, sizeof(buf));
        SNN_LOGI("stage %zu runs a fused plan: %s", i, buf);
    }
    // ---- independent neighbours: launching stage i and the launching stage k in front of it both read tensors that exist before k runs (i does not
    // consume k's output) -- the two branches of a residual block's entry.  Mark i: run() issues it on the side stream next to k.  One pair at a
    // time (k itself must not be the side stage of another pair).  Opt-in (SNN_BRANCH_OVERLAP=1): measured on ResNet-18 b32 the 1x1 stride-2
    // downsample (19 us alone) and the split-K 3x3 stride-2 convolution (53 us alone) do run concurrently (137 / 181 us summed over the three pairs
    // instead of 56 / 160) but each already fills the chip: 1.104 ms per step with the overlap, 1.101 ms without.
    // Round 6: when BOTH stages of such a pair run plans the library can put into one grid (snnhip_plan_groupable: conv2d_ksplit's 3x3 stride-2 convolution
    // and the 1x1 stride-2 downsample beside it), run() brackets them with a launch group instead -- one launch, the short blocks of the second behind the
    // first's; the default (SNN_STAGE_GROUPS=0: off).
    const char* overlap = getenv("SNN_BRANCH_OVERLAP");
    const char* groupsEnv = getenv("SNN_STAGE_GROUPS");
    const bool wantOverlap = overlap && atoi(overlap) != 0, wantGroups = !(groupsEnv && atoi(groupsEnv) == 0);
    if (!wantOverlap && !wantGroups) return;
    int prev = -1;
    for (size_t i = 0; i < stages.size(); ++i) {
        HipRenderPass* rp = passOf(i);
        if (!rp || rp->skip || !nodes[i].plan) {
            if (!stages[i].layer->isInputLayer && !(rp && rp->skip)) prev = -1; // an opaque stage: nothing pairs across it
            continue;
        }
        const int nIn = fused[i].plan ? fused[i].n_inputs : nodes[i].n_inputs;
        const int* ins = fused[i].plan ? fused[i].inputs : nodes[i].inputs;
        bool independent = prev >= 0 && !stages[static_cast<size_t>(prev)].sideOfPrevious && !stages[static_cast<size_t>(prev)].groupWithPrevious;
        for (int k = 0; k < nIn && independent; ++k) independent = ins[k] != prev;
        // the previous stage's fused group must not contain a producer of i either (a fused plan sits at the LAST stage of its group)
        for (int k = 0; k < nIn && independent; ++k)
            if (ins[k] >= 0 && ins[k] < prev && stages[static_cast<size_t>(ins[k])].fusedAway) independent = false;
        if (independent && i + 1 < stages.size()) { // (never the model's last stage: its output is bound to the caller)
            const snnhip_plan* pi = fused[i].plan ? fused[i].plan : nodes[i].plan;
            const snnhip_plan* pk = fused[static_cast<size_t>(prev)].plan ? fused[static_cast<size_t>(prev)].plan : nodes[static_cast<size_t>(prev)].plan;
            if (wantGroups && snnhip_plan_groupable(pi) && snnhip_plan_groupable(pk)) {
                stages[i].groupWithPrevious = true;
                SNN_LOGI("stage %zu (%s) and stage %d (%s) run in one launch group", i, stages[i].layer->name.c_str(), prev, stages[static_cast<size_t>(prev)].layer->name.c_str());
            } else if (wantOverlap) {
                stages[i].sideOfPrevious = true;
                SNN_LOGI("stage %zu (%s) runs beside stage %d (%s) on the side stream", i, stages[i].layer->name.c_str(), prev, stages[static_cast<size_t>(prev)].layer->name.c_str());
            }
        }
        prev = static_cast<int>(i);
    }
}

DeviceBackend* BackendBuilder::build(GpuContext* context, const InferenceGraph&) { // backendBuilder.cpp:36-58
    SNN_ASSERT(context);
    switch (context->backendType) {
    case GpuBackendType::HIP: return new HipBackend(context);
    default: SNN_CHK(false);
    }
    return nullptr;
}
