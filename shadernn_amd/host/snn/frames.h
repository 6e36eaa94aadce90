// snn/frames.h -- the resolved description of a model's frame ends (HIP extension; device-free: nothing here touches the GPU).  Every
// snn_model_create5..15 struct of include/snn_c.h resolves to ONE FrameSpec, and everything below the entry points -- createModel,
// MixedInferenceCore::CreationParameters, HipBackend::initFrames -- takes that one description.
#pragma once
#include <string>

#include "snn/inferencegraph.h"
#include "snn_c.h"

namespace snn {

struct FrameSpec {
    // the model's own end formats and maps: SNN_IO_FLOAT, or the 8- / 16-bit frame whose conversion joins the fusion graph (ESPCN folds it into its kernels)
    snn_frame_io2 model{SNN_IO_FLOAT, SNN_IO_FLOAT, {0, 0, 0, 0}, {1, 1, 1, 1}, {1, 1, 1, 1}, {0, 0, 0, 0}, 0, 65535, 0};
    // what the caller uploads: the model's frame, an RGB frame, luma + 4:2:0 chroma around a luma model, luma + 4:2:0 chroma of srcW x srcH in front of
    // an RGB(A) model (one launch into the model's float input tensor: snn_model_create14)
    enum class Source { MODEL, RGB, YUV420, YUV420_TENSOR } source = Source::MODEL;
    // what comes back: the model's frame, the merged RGB frame, luma + r-fold chroma, luma + chroma fitted to fitW x fitH, RGB from luma + chroma, luma + chroma from RGB,
    // the two RGB frames at fitW x fitH: from luma + chroma, merged with the colour frame that went in; and luma + 4:2:0 chroma of the model's own
    // extent from the output tensor of an RGB(A) model (one launch behind the model's last stage: snn_model_create15)
    enum class Sink { MODEL, RGB_MERGED, CHROMA_UP, FITTED, RGB_FROM_YUV, YUV420_FROM_RGB, RGB_FROM_YUV_FITTED, RGB_MERGED_FITTED, YUV420_FROM_TENSOR } sink = Sink::MODEL;
    int channels = 0;                                  // of the RGB end(s): 3 or 4
    bool wide = false;                                 // the video end's samples sit in 2-byte containers
    int maxval = 255, shift = 0;                       // ... with this depth and alignment (the chroma planes'; the luma plane's are model's)
    int siting = SNN_SITING_LEFT, range = SNN_RANGE_LIMITED;
    float kr = 0.299f, kb = 0.114f;                    // the matrix of the RGB end
    int fitW = 0, fitH = 0;                            // Sink::FITTED, Sink::RGB_FROM_YUV_FITTED, Sink::RGB_MERGED_FITTED
    bool planar = false;                               // the chroma planes are separate Cb and Cr planes (I420 / I010), not one interleaved CbCr plane
    int srcW = 0, srcH = 0, filter = SNN_FILTER_LINEAR; // Source::YUV420_TENSOR: the frame's extent, the sampler,
    float tensorMeans[3] = {0, 0, 0}, tensorNorms[3] = {1, 1, 1}, alpha = 1.0f; // ... and the normalisation of the input tensor
    // Sink::YUV420_FROM_TENSOR: the OUTPUT stream (the fields above stay the input end's: a video frame in front fills them as snn_model_create14 does)
    bool encWide = false, encPlanar = false;
    int encMaxval = 255, encShift = 0, encSiting = SNN_SITING_LEFT, encRange = SNN_RANGE_LIMITED;
    float encKr = 0.299f, encKb = 0.114f;
    float encScale[3] = {1, 1, 1}, encOffset[3] = {0, 0, 0}; // the output map: p = clamp(x * scale + offset, 0, encMaxval)
    const char* entry = "snn_model_create5";           // the entry point the request came through (log lines name it)
};

// One resolver per public struct (null for the float model of snn_model_create5 / 6): false = refused.  in_w x in_h x in_c and batch are the model input's.
bool resolveFrames(const snn_frame_io* io, int in_w, int in_h, int in_c, int batch, FrameSpec* spec);
bool resolveFrames(const snn_frame_io2* io, int in_w, int in_h, int in_c, int batch, FrameSpec* spec);
bool resolveFrames(const snn_colour_io* io, int in_w, int in_h, int in_c, int batch, FrameSpec* spec);
bool resolveFrames(const snn_video_io* io, int in_w, int in_h, int in_c, int batch, FrameSpec* spec);
bool resolveFrames(const snn_video_rgb_io* io, int in_w, int in_h, int in_c, int batch, FrameSpec* spec);
bool resolveFrames(const snn_encode_io* io, int in_w, int in_h, int in_c, int batch, FrameSpec* spec);
bool resolveFrames(const snn_fit_io* io, int in_w, int in_h, int in_c, int batch, FrameSpec* spec);
bool resolveFrames(const snn_planar_io* io, int in_w, int in_h, int in_c, int batch, FrameSpec* spec);
bool resolveFrames(const snn_rgb_fit_io* io, int in_w, int in_h, int in_c, int batch, FrameSpec* spec);
bool resolveFrames(const snn_video_tensor_io* io, int in_w, int in_h, int in_c, int batch, FrameSpec* spec);
bool resolveFrames(const snn_tensor_video_io* io, int in_w, int in_h, int in_c, int batch, FrameSpec* spec);
// ... by the number of the entry point, 5..15 (`io` is that entry point's struct)
bool resolveFrames(int entry, const void* io, int in_w, int in_h, int in_c, int batch, FrameSpec* spec);

// The rules that need the model's factor r, from the output desc of its last layer: a frame path around the model needs one channel out at r = 1..4
// times the input on both axes; luma + chroma from RGB r >= 2 and an even r * extent; a fitted size lies within [r * in / 2, r * in], and is
// no smaller than the colour frame that went in (logged); luma + chroma from the output tensor needs 3 or 4 channels out and an even extent (logged).
bool framesFitModel(const FrameSpec& spec, int in_w, int in_h, const InferenceGraph::IODesc& out);

ColorFormat frameColorFormat(int snnIoFormat); // SNN_IO_R8 .. SNN_IO_RGBA16 -> ColorFormat (NONE for SNN_IO_FLOAT and anything else)
int frameIoFormat(ColorFormat f);              // ... and back (SNN_IO_FLOAT for what is no frame format)

std::string formatFrameSpec(const FrameSpec& spec); // one canonical line: "<the model part> | <the frame ends> | entry=<name>"

} // namespace snn
