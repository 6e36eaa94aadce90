// ic2/backend.h -- DeviceBackend / RenderPass / InferencePass (reference core/src/ic2/backend.h:32-91, renderpass.h:24-67,
// inferencepass.h:31-62) and the HIP implementations that sit on the C-ABI of include/snnhip.h.
#pragma once
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "snn/core.h"
#include "snn/deviceTimer.h"
#include "snn/imageTexture.h"

struct snnhip_plan;
struct snnhip_ctx;

namespace snn {

class RenderPass {
public:
    RenderPass() = default;
    virtual ~RenderPass() = default;
    SNN_NO_COPY(RenderPass);
    virtual bool debugPassOutput(const std::string&) { return true; }
    virtual bool debugPassInputs(const std::string&) { return true; }
    virtual bool debugPassWeights(const std::string&, int) { return true; }
    virtual void run() {}
};

// One inference pass = what the layer's createCS() produced.  The Vulkan flavour carries SPIR-V + specialisation constants
// (inferencepassVulkan.h:27-41); the HIP flavour carries an executable plan (device-resident weights + launch recipe).
struct InferencePass {
    std::string source; // operator description (the reference stores the shader asset name here)
    // Host-side recipe: packed descriptor + weights captured by value.  The backend turns it into device resources in
    // initRenderPasses(), exactly where VulkanRenderPass's constructor builds the pipeline and uploads the weight image.
    std::function<int(snnhip_ctx*, snnhip_plan**)> createPlan;
};
struct InferencePasses {
    std::vector<InferencePass> passes;
};
typedef std::shared_ptr<InferencePasses> InferencePassesSptr;

namespace dp {

class GenericModelLayer;

class DeviceBackend {
public:
    DeviceBackend() = default;
    virtual ~DeviceBackend() = default;
    SNN_NO_COPY(DeviceBackend);
    virtual void initRenderPasses(GenericModelLayer*, ImageTextureArrayAccessor, ImageTextureArrayAccessor) {}
    virtual void prepareRun(MixedInferenceCore::RunParameters&, RenderStagesArray&, bool, uint32_t) {}
    virtual void prepareStage(MixedInferenceCore::RunParameters&, RenderStage&) {}
    virtual void postRun(RenderStagesArray&, bool, const std::string&) {}
    virtual bool sync() { return false; }
    virtual void cleanupRun() {}
    virtual DeviceTimer* createDeviceTimer(const std::string&) { return nullptr; }
    virtual bool isProfilingEnabled(bool = false) { return true; }
    // HIP extension, called once after every stage is initialised: may replace linear runs of passes by fused plans
    virtual void finalizeStages(RenderStagesArray&, bool /*dumpOutputs*/, bool /*fuseChains*/) {}
    // HIP extension: record the launches of one inference once and replay them (the counterpart of the Vulkan backend recording a command
    // buffer, vulkanBackend.cpp:80-95).  beginRecord returns false when the backend cannot record; replay re-submits the last recording.
    virtual bool beginRecord() { return false; }
    virtual bool endRecord() { return false; }
    virtual bool replay() { return false; }
    virtual void dropRecording() {}
    // HIP extension: two independent stages side by side.  forkSide: what runs next goes to a second stream that starts behind the work enqueued
    // so far; backToMain: what runs next goes to the main stream again; joinSide: the main stream waits for the side stream.
    virtual bool forkSide() { return false; }
    virtual void backToMain() {}
    virtual void joinSide() {}
    // HIP extension: a launch group -- groupable plans run between the two calls are launched by groupEnd, two compatible ones as one kernel launch
    virtual bool groupBegin() { return false; }
    virtual void groupEnd() {}
};

class HipRenderPass : public RenderPass {
public:
    HipRenderPass(snnhip_plan* p, ImageTexture* in, ImageTexture* out, const std::string& layerName, bool ownsPlan = false)
        : plan(p), input(in), output(out), name(layerName), owns(ownsPlan) {}
    std::vector<ImageTexture*> extraInputs; // inputs 1.. of multi-input operators (Add: addlayerVulkan.cpp:98 binds uInput0, uInput1)
    ~HipRenderPass() override;
    void run() override;                                   // enqueue only (vulkanRenderpass.cpp:257-259 records Dispatch + barrier)
    bool debugPassOutput(const std::string& folder) override; // "<folder>/<layer name> pass[0].dump" (vulkanBackend.cpp:132-134)
    bool debugPassInputs(const std::string& folder) override; // "<layer name> pass[0]_input.dump" (vulkanRenderpass.cpp:262-277)
    snnhip_plan* plan;
    ImageTexture *input, *output;
    std::string name;
    bool owns;
    bool skip = false; // fused into an earlier pass
    const snnhip_tensor* rawInput = nullptr; // HIP extension: the 8-bit input frame a fused plan reads instead of `input` (rule A8)
    snnhip_tensor* rawOutput = nullptr;      // ... and the 8-bit output frame it writes instead of `output` (rule B8)
};

class HipBackend : public DeviceBackend {
public:
    explicit HipBackend(GpuContext* context);
    void initRenderPasses(GenericModelLayer* layer, ImageTextureArrayAccessor in, ImageTextureArrayAccessor out) override;
    void postRun(RenderStagesArray& stages, bool dumpOutput, const std::string& folder) override;
    bool sync() override; // hipStreamSynchronize == QueueSubmitAndWait (vulkanBackend.cpp:97-106)
    DeviceTimer* createDeviceTimer(const std::string& name) override;
    void finalizeStages(RenderStagesArray& stages, bool dumpOutputs, bool fuseChains) override;
    bool beginRecord() override;
    bool endRecord() override;
    bool replay() override;
    void dropRecording() override;
    bool forkSide() override;
    void backToMain() override;
    void joinSide() override;
    bool groupBegin() override;
    void groupEnd() override;
    // 8-bit frame I/O (MixedInferenceCore::CreationParameters::outputFormat / inputsDesc[0].format): called before finalizeStages.  The conversion
    // plans become nodes of the fusion graph; runFrameIn / runFrameOut launch whatever was not folded into a stage's fused plan.
    // in16 / out16: that end is a 16-bit frame (u16 plans, SNNHIP_U16 tensor) with the container layout inShift / outMaxval, outShift.
    void initFrameIO(bool in, bool out, int n, int inH, int inW, int inC, int outH, int outW, int outC, int dtype, const float means[4],
                     const float norms[4], const float scale[4], const float offset[4], bool in16 = false, bool out16 = false, int inShift = 0,
                     int outMaxval = 65535, int outShift = 0);
    void runFrameIn(const ImageTexture& modelInput);
    void runFrameOut(const ImageTexture& lastOutput);
    // colour frames around a luma-only model (CreationParameters::colourChannels): called after initFrameIO with R8 frames at both ends.  The luma
    // plan fills the model's input frame from the colour frame in runFrameIn, the merge plan builds the colour output frame from the model's output
    // frame and the colour frame in runFrameOut: two launches more on the context's stream, in front of and behind everything else of an inference.
    void initColourIO(int channels, float kr, float kb);
    int colourLaunches() const { return (lumaPlan ? 1 : 0) + (mergePlan ? 1 : 0); }
    std::string describeColour() const; // one line per extra launch (empty without colour frames)
    // NV12 / P010 video frames around a luma-only model (CreationParameters::videoDtype): called after initFrameIO with R8 / R16 frames at both
    // ends.  The luma plane IS the model's frame; the chroma plan upsamples the CbCr plane [n][H/2][W/2][2] to [n][rH/2][rW/2][2] in runFrameOut,
    // one launch more on the context's stream behind everything else of an inference (a straight line: no side stream, no parallel graph branch).
    void initVideoIO(int dtype, int maxval, int shift, int siting, bool planar = false);
    // ... or to packed RGB (CreationParameters::videoRgbChannels): the yuv_rgb plan builds the RGB / RGBA output frame [n][rH][rW][channels] from the
    // model's output luma frame and the ORIGINAL CbCr plane in runFrameOut, in the chroma launch's place (no chroma plan, no upscaled chroma plane)
    void initVideoRgbIO(int dtype, int maxval, int shift, int siting, int channels, int range, float kr, float kb, bool planar = false);
    // ... or to an NV12 / P010 frame of any size between half and all of the model's output (CreationParameters::fitW / fitH): two plane_fit plans in
    // runFrameOut, the model's output luma frame to [n][outH][outW][1] and the ORIGINAL CbCr plane to [n][outH/2][outW/2][2] (no chroma plan)
    void initVideoFitIO(int dtype, int maxval, int shift, int siting, int outW, int outH, bool planar = false);
    // RGB8 / RGBA8 frames in, an NV12 frame out (CreationParameters::encodeChannels): called after initFrameIO with R8 frames at both ends.  The luma
    // plan of initColourIO fills the model's input frame in runFrameIn; the model's output frame IS the NV12 frame's luma plane; the rgb_cbcr plan
    // builds its chroma plane [n][rH/2][rW/2][2] from the colour input frame in runFrameOut (no merge plan, no colour output frame)
    void initEncodeIO(int channels, int siting, int range, float kr, float kb, bool planar = false);
    // `planar` on the four above (CreationParameters::videoPlanar, I420 / I010): the chroma tensors are [2n][h][w][1], plane 2k = Cb and 2k + 1 = Cr of
    // frame k; chroma_up and plane_fit run with C = 1 over the 2n planes, yuv_rgb and rgb_cbcr as snnhip_yuv_rgb_planar_plan_create /
    // snnhip_rgb_cbcr_planar_plan_create.  The launches are the same in number and place
    bool planarVideo() const { return planarChroma; }
    bool encodeOutput() const { return cbcrPlan != nullptr; }
    int videoLaunches() const { return fitLumaPlan ? 2 : chromaPlan || yuvRgbPlan || cbcrPlan ? 1 : 0; }
    std::string describeVideo() const; // one line for every extra launch (empty without video frames)
    snnhip_tensor* chromaInput() const { return chromaInT; }
    snnhip_tensor* chromaOutput() const { return chromaOutT; }
    snnhip_tensor* frameInput() const { return colourInT ? colourInT : frameInT; }
    snnhip_tensor* frameOutput() const { return fitLumaT ? fitLumaT : rgbOutT ? rgbOutT : colourOutT ? colourOutT : frameOutT; }

private:
    snnhip_plan *frameInPlan = nullptr, *frameOutPlan = nullptr; // owned
    snnhip_tensor *frameInT = nullptr, *frameOutT = nullptr;      // owned, SNNHIP_U8 or SNNHIP_U16
    bool frameInFused = false, frameOutFused = false;
    snnhip_plan *lumaPlan = nullptr, *mergePlan = nullptr;   // owned
    snnhip_tensor *colourInT = nullptr, *colourOutT = nullptr; // owned, SNNHIP_U8 [n][H][W][C] / [n][rH][rW][C]
    snnhip_plan* chromaPlan = nullptr;                          // owned
    snnhip_tensor *chromaInT = nullptr, *chromaOutT = nullptr;  // owned, SNNHIP_U8 / SNNHIP_U16 [n][H/2][W/2][2] / [n][rH/2][rW/2][2]
    snnhip_plan* yuvRgbPlan = nullptr;                          // owned
    snnhip_tensor* rgbOutT = nullptr;                           // owned, SNNHIP_U8 / SNNHIP_U16 [n][rH][rW][3 or 4]
    snnhip_plan* cbcrPlan = nullptr;                            // owned (its output is chromaOutT, its input colourInT)
    snnhip_plan *fitLumaPlan = nullptr, *fitChromaPlan = nullptr; // owned (the chroma plan runs chromaInT -> chromaOutT)
    snnhip_tensor* fitLumaT = nullptr;                          // owned, SNNHIP_U8 / SNNHIP_U16 [n][outH][outW][1]
    bool planarChroma = false;                                  // chromaInT / chromaOutT are [2n][h][w][1]
    snnhip_ctx* ctx;
    std::vector<snnhip_plan*> chainPlans; // owned
    void* recording = nullptr;            // snnhip_graph* of the last recorded inference
    std::vector<std::shared_ptr<RenderPass>> replacedPasses; // their plans may still be referenced by a chain (unfused steps)
public:
    ~HipBackend() override;
};

struct BackendBuilder {
    static DeviceBackend* build(GpuContext* context, const InferenceGraph& ig); // backendBuilder.cpp:36-58
};

} // namespace dp
} // namespace snn
