// snn/core.h -- MixedInferenceCore / RenderStage (reference core/inc/snn/core.h:37-146).
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "snn/deviceTimer.h"
#include "snn/frames.h"
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
        bool halfTensors = false; // the model's tensors are fp16 (preferHp): the frame conversions read / write halfs
        // HIP extension: the frames at the model's ends (snn/frames.h; the default is none: float tensors in and out).  frames.model names 8- / 16-bit
        // frames of the model's own channel count (inputsDesc[0].format is the same format as a ColorFormat): their conversions join the stage graph
        // handed to snnhip_graph_fuse, so the chain rules can fold them into fused kernels (ESPCN: rules A8 / B8); otherwise -- and always with dumps --
        // they run as launches of their own.  frames.source / sink name colour or video frames around a luma-only model: launches in front of and
        // behind the model's on the same stream (HipBackend::initFrames)
        FrameSpec frames;
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
    bool planarOutput() const; // ... the output's: planarVideo(), or the output stream's own layout behind [tensor yuv] (snn_model_create15)
    bool encodeOutput() const; // the output is the 4:2:0 frame of snn_model_create10 / 15: frameOutput() its luma plane, chromaOutput() its chroma
    const FrameSpec& frames() const { return cp.frames; } // the resolved description the model was built from (snn_model_reference_frame reads the output's depth)

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
