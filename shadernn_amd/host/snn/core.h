// snn/core.h -- MixedInferenceCore / RenderStage (reference core/inc/snn/core.h:37-146).
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "snn/deviceTimer.h"
#include "snn/inferencegraph.h"
#include "snn/layeroption.h"
#include "snn/snn.h"

struct snnhip_tensor;
namespace snn {
namespace dp {
class DeviceBackend;
class HipBackend;
}
typedef enum class Transition { Backend_CPU_GPU, Backend_GPU_CPU, NOT_DEFINED = 200 } Transition;

struct RenderStage {
    explicit RenderStage(GpuContext* context) : stageInputs(context), stageOutputs(context) {}
    std::shared_ptr<InferenceGraph::Layer> layer;
    bool flattenLayer = false;
    std::shared_ptr<DeviceTimer> timer;
    Backend backend = Backend::Backend_GPU;
    Transition transition = Transition::NOT_DEFINED;
    ImageTextureArray stageInputs;
    ImageTextureArray stageOutputs;
    std::vector<int> inputIds;
    std::vector<int> delayBindMask;
    bool fusedAway = false; // HIP extension: this stage's work is done by the fused plan of a later stage (HipBackend::finalizeStages)
    // HIP extension (HipBackend::finalizeStages): this stage and the previous launching stage read only tensors produced earlier -- two
    // branches of a residual block (ResNet: the 3x3 stride-2 convolution and the 1x1 stride-2 downsample of the same input).  run() issues this
    // one on the backend's side stream next to the previous one instead of behind it (DeviceBackend::forkSide / joinSide).
    bool sideOfPrevious = false;
    // ... or, when both stages run plans the library can launch as ONE grid (snnhip_plan_groupable: the K-split convolutions), inside a launch group
    // (DeviceBackend::groupBegin / groupEnd): the default for such pairs; SNN_STAGE_GROUPS=0 switches it off
    bool groupWithPrevious = false;
};
typedef std::vector<RenderStage> RenderStagesArray;

class MixedInferenceCore {
public:
    virtual ~MixedInferenceCore();
    SNN_NO_COPY(MixedInferenceCore);
    struct RunParameters {
        ImageTextureArray* inputImages = nullptr;
        ImageTextureArray* outputImages = nullptr;
        std::vector<std::vector<std::vector<float>>> inputMatrix;
        std::vector<std::vector<std::vector<float>>> output;
        SNNModelOutput modelOutput;
        // HIP extension: return right after the inference is enqueued instead of waiting for it (the reference waits once per inference,
        // core.cpp:203).  The caller keeps several inferences in flight on the backend's stream and calls sync() when it needs a result;
        // ignored with profiling / dumps / CPU stages / a classifier or detection output (those read results on the host inside run()).
        bool deferSync = false;
    };
    void run(RunParameters& rp);
    bool sync(); // HIP extension: wait for every inference enqueued with deferSync
    struct CreationParameters : InferenceGraph {
        uint32_t outputWidth = 0, outputHeight = 0, outputDepth = 0;
        bool dumpOutputs = false;
        bool fuseChains = true;
        bool profiling = false; // the reference enables per-stage timers at compile time (-DPROFILING, CMakeLists.txt:44-46)
        // HIP extension: record the launch sequence of the first run() as a hipGraph and replay it while the caller keeps feeding the same input
        // textures (re-recorded when they change).  Ignored with dumpOutputs / profiling / CPU stages (those need the host between launches).
        bool captureGraph = false;
        // HIP extension: 8-bit frames at the model's ends (inputsDesc[0].format / outputFormat R8, RGB8 or RGBA8, channel count = the model's own).
        // The conversions (snnhip_u8_in_plan_create / _u8_out_plan_create) join the stage graph handed to snnhip_graph_fuse, so the chain rules can
        // fold them into fused kernels (ESPCN: rules A8 / B8); otherwise -- and always with dumps -- they run as launches of their own.
        ColorFormat outputFormat = ColorFormat::RGBA32F;
        float frameInMeans[4] = {0, 0, 0, 0}, frameInNorms[4] = {1, 1, 1, 1};
        float frameOutScale[4] = {1, 1, 1, 1}, frameOutOffset[4] = {0, 0, 0, 0};
        // 16-bit frames (R16, RGB16, RGBA16: snnhip_u16_in_plan_create / _u16_out_plan_create, handled exactly as the 8-bit ones): the container's
        // layout.  Low-aligned 10 / 12-bit: maxval 1023 / 4095, shifts 0; P010-style high-aligned 10-bit: maxval 1023, shifts 6; full 16-bit: 65535.
        int frameInShift = 0, frameOutMaxval = 65535, frameOutShift = 0;
        bool halfTensors = false; // the model's tensors are fp16 (preferHp): the conversions read / write halfs
        // HIP extension: colour frames around a luma-only model (snn_model_create7).  colourChannels 3 / 4 = RGB8 / RGBA8 frames at both ends of a model
        // whose own ends are R8 frames: run() puts snnhip_rgb_luma_plan_create's launch in front of the model and snnhip_ycc_merge_plan_create's behind it
        int colourChannels = 0;
        float colourKr = 0.299f, colourKb = 0.114f;
        // HIP extension: NV12 / P010 video frames around a luma-only model (snn_model_create8).  videoDtype SNNHIP_U8 / SNNHIP_U16 (0 = none): the
        // model's own ends are R8 / R16 frames; run() puts snnhip_chroma_up_plan_create's launch on the half-resolution CbCr plane behind the model
        int videoDtype = 0, videoMaxval = 255, videoShift = 0, videoSiting = 1;
        // ... or, with videoRgbChannels 3 / 4 (snn_model_create9), snnhip_yuv_rgb_plan_create's launch instead: the model's output luma frame and the
        // original CbCr plane to an RGB / RGBA frame (videoRange SNNHIP_RANGE_*, matrix videoKr / videoKb)
        int videoRgbChannels = 0, videoRange = 0;
        // ... or, with fitW / fitH (snn_model_create11), two snnhip_plane_fit_plan_create launches instead: the model's output luma frame and the
        // original CbCr plane resampled to an NV12 / P010 frame of fitW x fitH (no chroma_up launch)
        int fitW = 0, fitH = 0;
        float videoKr = 0.299f, videoKb = 0.114f;
        // HIP extension: RGB8 / RGBA8 frames in, an NV12 frame out around a luma-only model (snn_model_create10).  encodeChannels 3 / 4: run() puts
        // snnhip_rgb_luma_plan_create's launch in front of the model, as colourChannels does, and snnhip_rgb_cbcr_plan_create's behind it, from the
        // colour input frame to the output frame's chroma plane (encodeSiting SNNHIP_SITING_*, encodeRange SNNHIP_RANGE_*, matrix colourKr / colourKb)
        int encodeChannels = 0, encodeSiting = 1, encodeRange = 0;
        // HIP extension: planar 4:2:0 frames (I420 / I010, snn_model_create12) on the video end(s) of any of the four paths above: the chroma tensors
        // are [2 * batch][h][w][1] (plane 2n = Cb, 2n + 1 = Cr of frame n) instead of [batch][h][w][2]; chroma_up and plane_fit run with C = 1 over
        // the 2 * batch planes, yuv_rgb and rgb_cbcr as their planar plans.  The same number of launches; no interleaving launch anywhere
        bool videoPlanar = false;
    };
    static std::unique_ptr<MixedInferenceCore> create(GpuContext* context, const CreationParameters& cp);
    static std::unique_ptr<MixedInferenceCore> create(GpuContext* context, const std::string& modelFileName, const dp::ShaderGenOptions& options,
                                                      bool dumpOutputs = false);
    void writeTimeStat(std::map<std::string, std::vector<double>>& timeArray);
    size_t numStages() const { return stages.size(); }
    RenderStage& stage(size_t i) { return stages[i]; }
    std::string describe() const; // HIP extension: which kernel variant each stage runs
    // HIP extension: run the next inferences launch by launch even when a recording exists (per-launch profiling needs the plans to run)
    void suspendReplay(bool suspend) { replaySuspended = suspend; }
    // HIP extension: the model's input / output frame tensors (SNNHIP_U8 or SNNHIP_U16 [batch][H][W][C]; null without frame I/O at that end)
    snnhip_tensor* frameInput() const;
    snnhip_tensor* frameOutput() const;
    snnhip_tensor* chromaInput() const; // the CbCr planes of a video model (snn_model_create8), null otherwise
    snnhip_tensor* chromaOutput() const;
    bool planarVideo() const;  // the chroma tensors are planar [2 * batch][h][w][1] (snn_model_create12)
    bool encodeOutput() const; // the output is the NV12 frame of snn_model_create10: frameOutput() its luma plane, chromaOutput() its CbCr plane

private:
    GpuContext* context;
    bool bindOutput = true;
    CreationParameters cp;
    RenderStagesArray stages;
    dp::DeviceBackend* backend = nullptr;
    dp::HipBackend* frameBackend = nullptr; // set when the model has an 8-bit input or output frame
    DeviceTimer* gpuRunTime = nullptr;
    struct InputKey { // what a recorded launch sequence depends on: the device buffer (address), its extent and element type
        const void* data;
        int dims[4];
        int dtype;
        bool operator==(const InputKey& o) const {
            return data == o.data && dims[0] == o.dims[0] && dims[1] == o.dims[1] && dims[2] == o.dims[2] && dims[3] == o.dims[3] && dtype == o.dtype;
        }
    };
    std::vector<InputKey> recordedInputs; // device buffers the recording reads (delay-bound model inputs)
    bool graphUsable = false;
    bool replaySuspended = false;
    Timer cpuRunTime = Timer("IC2 Total CPU Runtime");
    explicit MixedInferenceCore(GpuContext* context_);
    bool init(const CreationParameters& cp);
};
} // namespace snn
