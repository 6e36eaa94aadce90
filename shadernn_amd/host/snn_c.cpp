// snn_c.cpp -- C binding of the host mirror for tests / harnesses (see include/snn_c.h).
#include <cstring>
#include <vector>

#include "../../include/snn_c.h"
#include "../../include/snnhip.h"
#include "ic2/backend.h"
#include "ic2/dp.h"
#include "ic2/json.h"
#include "ic2/layerFactory.h"
#include "snn/contextFactory.h"
#include "snn/core.h"
#include "snn/frames.h"
#include "snn/planes.h"

using namespace snn;

struct snn_model {
    GpuContext* context = nullptr;
    std::unique_ptr<MixedInferenceCore> core;
    ImageTextureArray inputs{nullptr};
    ImageTextureArray outputs{nullptr};
    int inW = 0, inH = 0, inC = 0, batch = 1;
    bool half = false;
    bool videoTensor = false; // snn_model_create14: the input tensor is written by the [yuv tensor] launch, never by an upload of floats or bytes
    SNNModelOutput modelOutput;
    std::vector<char> staging; // host buffer of snn_model_upload_frame_planes / _download_frame_planes for planes that are not tight and adjacent
    // frame quality against a ground-truth frame (snn_model_reference_frame / _frame_metrics): one per output plane tensor, made by the first reference
    struct MetricsEnd {
        snnhip_tensor* ref = nullptr;    // the reference plane(s), the output tensor's extent and dtype
        snnhip_tensor* result = nullptr; // F32 [n][1][c][2], the plan's own output
        snnhip_plan* plan = nullptr;
        int maxval = 255;
    };
    MetricsEnd metricsFrame, metricsChroma; // the output frame (or its luma plane), the chroma plane(s) of a video output
    bool referenceSet = false;
};

static dp::ShaderGenOptions makeOptions(int w, int h, int c, bool fuse, bool half = false, int batch = 1) {
    dp::ShaderGenOptions sgo;
    const ColorFormat fmt = half ? ColorFormat::RGBA16F : ColorFormat::RGBA32F;
    InferenceGraph::IODesc in{fmt, static_cast<uint32_t>(w), static_cast<uint32_t>(h), static_cast<uint32_t>(UP_DIV(c, 4)), static_cast<uint32_t>(c)};
    sgo.desiredInput.push_back(in);
    sgo.desiredOutputFormat = fmt;
    sgo.preferrHalfPrecision = half;
    sgo.compute = true;
    sgo.fuseChains = fuse;
    sgo.batch = static_cast<uint32_t>(batch);
    return sgo;
}

static void makeIO(snn_model* m, bool half = false) {
    m->inputs = ImageTextureArray(m->context);
    m->outputs = ImageTextureArray(m->context);
    m->inputs.push_back(ImageTextureFactory::createImageTexture(m->context, {static_cast<uint32_t>(m->inW), static_cast<uint32_t>(m->inH),
                                                                             static_cast<uint32_t>(UP_DIV(m->inC, 4)), static_cast<uint32_t>(m->batch)},
                                                                half ? ColorFormat::RGBA16F : ColorFormat::RGBA32F, nullptr, static_cast<uint32_t>(m->inC)));
    m->outputs.allocate(1);
}

extern "C" {

// what every snn_model_create* takes beside its frame struct
struct ModelArgs {
    const char* json_path;
    int device, in_w, in_h, in_c, dump_outputs, fuse_chains, profiling, prefer_half, capture_graph, batch;
    snn_model** out;
};

static int createModel(const ModelArgs& a, const FrameSpec& spec) {
    if (!a.json_path || !a.out) return -1;
    const bool half = a.prefer_half != 0;
    auto* m = new snn_model();
    // C++ exceptions (std::bad_alloc, a parser's std::out_of_range, ...) must not unwind through the C boundary: report -2 and free what was built.
    // (SNN_RIP is the reference's abort-on-fatal-error convention, utils.h:57-62: it terminates the process and is not an exception.)
    try {
        m->batch = a.batch;
        m->context = createHipContext(a.device);
        m->inW = a.in_w;
        m->inH = a.in_h;
        m->inC = a.in_c;
        dp::ShaderGenOptions sgo = makeOptions(a.in_w, a.in_h, a.in_c, a.fuse_chains != 0, half, a.batch);
        if (spec.model.in_format != SNN_IO_FLOAT) sgo.desiredInput[0].format = frameColorFormat(spec.model.in_format);
        if (spec.model.out_format != SNN_IO_FLOAT) sgo.desiredOutputFormat = frameColorFormat(spec.model.out_format);
        auto layers = dp::loadFromJsonModel(a.json_path, false, sgo.mrtMode, sgo.weightMode, half); // preferHp: weights truncated to fp16 (Q13)
        MixedInferenceCore::CreationParameters cp;
        static_cast<InferenceGraph&>(cp) = dp::generateInferenceGraph(layers, sgo);
        cp.dumpOutputs = a.dump_outputs != 0;
        cp.fuseChains = a.fuse_chains != 0;
        cp.profiling = a.profiling != 0;
        cp.captureGraph = a.capture_graph != 0;
        cp.halfTensors = half;
        cp.frames = spec;
        if (!framesFitModel(spec, a.in_w, a.in_h, cp.layers.back()->outputDesc)) { // (refused here, before anything is built on the device)
            snn_model_destroy(m);
            return -1;
        }
        m->core = MixedInferenceCore::create(m->context, cp);
        makeIO(m, half);
        m->half = half;
        m->videoTensor = spec.source == FrameSpec::Source::YUV420_TENSOR;
    } catch (const std::exception& e) {
        SNN_LOGE("snn_model_create: %s", e.what());
        snn_model_destroy(m);
        return -2;
    } catch (...) {
        snn_model_destroy(m);
        return -2;
    }
    *a.out = m;
    return 0;
}

// snn_model_create<entry>: `io` is that entry point's struct, resolved to the one description everything below takes (snn/frames.h)
static int create(const ModelArgs& a, int entry, const void* io) {
    FrameSpec spec;
    if (!resolveFrames(entry, io, a.in_w, a.in_h, a.in_c, a.batch, &spec)) return -1;
    return createModel(a, spec);
}

int snn_frames_resolve(int entry, const void* io, int in_w, int in_h, int in_c, int batch, char* buf, int buflen) {
    FrameSpec spec;
    if (!resolveFrames(entry, io, in_w, in_h, in_c, batch, &spec)) return -1;
    if (buf && buflen > 0) snprintf(buf, static_cast<size_t>(buflen), "%s", formatFrameSpec(spec).c_str());
    return 0;
}

int snn_model_create(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                     snn_model** out) {
    return create({json_path, device, in_w, in_h, in_c, dump_outputs, fuse_chains, profiling, 0, 0, 1, out}, 5, nullptr);
}

int snn_model_create2(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                      int prefer_half, snn_model** out) {
    return create({json_path, device, in_w, in_h, in_c, dump_outputs, fuse_chains, profiling, prefer_half, 0, 1, out}, 5, nullptr);
}

int snn_model_create3(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                      int prefer_half, int capture_graph, snn_model** out) {
    return create({json_path, device, in_w, in_h, in_c, dump_outputs, fuse_chains, profiling, prefer_half, capture_graph, 1, out}, 5, nullptr);
}

int snn_model_create4(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                      int prefer_half, int capture_graph, int batch, snn_model** out) {
    return create({json_path, device, in_w, in_h, in_c, dump_outputs, fuse_chains, profiling, prefer_half, capture_graph, batch, out}, 5, nullptr);
}

int snn_model_create5(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                      int prefer_half, int capture_graph, int batch, const snn_frame_io* io, snn_model** out) {
    return create({json_path, device, in_w, in_h, in_c, dump_outputs, fuse_chains, profiling, prefer_half, capture_graph, batch, out}, 5, io);
}

int snn_model_create6(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                      int prefer_half, int capture_graph, int batch, const snn_frame_io2* io, snn_model** out) {
    return create({json_path, device, in_w, in_h, in_c, dump_outputs, fuse_chains, profiling, prefer_half, capture_graph, batch, out}, 6, io);
}

int snn_model_create7(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                      int prefer_half, int capture_graph, int batch, const snn_colour_io* io, snn_model** out) {
    return create({json_path, device, in_w, in_h, in_c, dump_outputs, fuse_chains, profiling, prefer_half, capture_graph, batch, out}, 7, io);
}

int snn_model_create8(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                      int prefer_half, int capture_graph, int batch, const snn_video_io* io, snn_model** out) {
    return create({json_path, device, in_w, in_h, in_c, dump_outputs, fuse_chains, profiling, prefer_half, capture_graph, batch, out}, 8, io);
}

int snn_model_create9(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                      int prefer_half, int capture_graph, int batch, const snn_video_rgb_io* io, snn_model** out) {
    return create({json_path, device, in_w, in_h, in_c, dump_outputs, fuse_chains, profiling, prefer_half, capture_graph, batch, out}, 9, io);
}

int snn_model_create10(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                       int prefer_half, int capture_graph, int batch, const snn_encode_io* io, snn_model** out) {
    return create({json_path, device, in_w, in_h, in_c, dump_outputs, fuse_chains, profiling, prefer_half, capture_graph, batch, out}, 10, io);
}

int snn_model_create11(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                       int prefer_half, int capture_graph, int batch, const snn_fit_io* io, snn_model** out) {
    return create({json_path, device, in_w, in_h, in_c, dump_outputs, fuse_chains, profiling, prefer_half, capture_graph, batch, out}, 11, io);
}

int snn_model_create12(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                       int prefer_half, int capture_graph, int batch, const snn_planar_io* io, snn_model** out) {
    return create({json_path, device, in_w, in_h, in_c, dump_outputs, fuse_chains, profiling, prefer_half, capture_graph, batch, out}, 12, io);
}

int snn_model_create13(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                       int prefer_half, int capture_graph, int batch, const snn_rgb_fit_io* io, snn_model** out) {
    return create({json_path, device, in_w, in_h, in_c, dump_outputs, fuse_chains, profiling, prefer_half, capture_graph, batch, out}, 13, io);
}

int snn_model_create14(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                       int prefer_half, int capture_graph, int batch, const snn_video_tensor_io* io, snn_model** out) {
    return create({json_path, device, in_w, in_h, in_c, dump_outputs, fuse_chains, profiling, prefer_half, capture_graph, batch, out}, 14, io);
}

int snn_model_create15(const char* json_path, int device, int in_w, int in_h, int in_c, int dump_outputs, int fuse_chains, int profiling,
                       int prefer_half, int capture_graph, int batch, const snn_tensor_video_io* io, snn_model** out) {
    FrameSpec spec;
    if (!resolveFrames(15, io, in_w, in_h, in_c, batch, &spec)) { // (what the model file decides is framesFitModel's to refuse and to log)
        if (!io) SNN_LOGE("snn_model_create15: null struct");
        else SNN_LOGE("snn_model_create15: the request was refused (formats 0x%x -> 0x%x, maxval %d, shift %d, siting %d, range %d, kr %g, kb %g, input %dx%dx%d, batch %d)",
                      io->in_format, io->out_format, io->maxval, io->shift, io->siting, io->range, io->kr, io->kb, in_w, in_h, in_c, batch);
        return -1;
    }
    return createModel({json_path, device, in_w, in_h, in_c, dump_outputs, fuse_chains, profiling, prefer_half, capture_graph, batch, out}, spec);
}

// one plane of every frame between the caller's interleaved frames and a contiguous device tensor; `stride` and `offset` in bytes within a frame
static int movePlane(snnhip_tensor* t, int batch, char* frames, size_t stride, size_t offset, bool upload) {
    const size_t total = snnhip_tensor_bytes(t), plane = total / static_cast<size_t>(batch);
    if (batch == 1) return (upload ? snnhip_tensor_upload_raw(t, frames + offset, total) : snnhip_tensor_download_raw(t, frames + offset, total)) == SNNHIP_OK ? 0 : -1;
    std::vector<char> staging(total);
    if (upload) {
        for (int n = 0; n < batch; ++n) memcpy(staging.data() + n * plane, frames + n * stride + offset, plane);
        return snnhip_tensor_upload_raw(t, staging.data(), total) == SNNHIP_OK ? 0 : -1;
    }
    if (snnhip_tensor_download_raw(t, staging.data(), total) != SNNHIP_OK) return -1;
    for (int n = 0; n < batch; ++n) memcpy(frames + n * stride + offset, staging.data() + n * plane, plane);
    return 0;
}

static int moveVideoFrames(snn_model* m, void* frames, bool upload) {
    if (!m || !frames || !m->core) return -1;
    snnhip_tensor* y = upload ? m->core->frameInput() : m->core->frameOutput();
    snnhip_tensor* c = upload ? m->core->chromaInput() : m->core->chromaOutput();
    if (!y || !c || (upload ? m->core->planarVideo() : m->core->planarOutput())) return -1; // (planar ends: snn_model_upload_frame_planes / _download_frame_planes)
    const size_t yb = snnhip_tensor_bytes(y) / static_cast<size_t>(m->batch), cb = snnhip_tensor_bytes(c) / static_cast<size_t>(m->batch);
    char* p = static_cast<char*>(frames);
    if (movePlane(y, m->batch, p, yb + cb, 0, upload) != 0) return -1;
    return movePlane(c, m->batch, p, yb + cb, yb, upload);
}

int snn_model_upload_frame_nv12(snn_model* m, const void* frames) { return moveVideoFrames(m, const_cast<void*>(frames), true); }

int snn_model_download_frame_nv12(snn_model* m, void* frames) { return moveVideoFrames(m, frames, false); }

// `pieces` (one plane of one frame each: `rows` rows of `rowBytes` bytes, pitch[i] bytes apart, in the order the dense device tensor t holds them)
// between the caller's memory and t.  Tight, adjacent pieces are one run of memory: copied straight.  Anything else goes through the model's staging
// buffer row by row; only the rows' own bytes are read or written, never the padding between them
static int movePieces(snn_model* m, snnhip_tensor* t, const std::vector<char*>& pieces, const std::vector<size_t>& pitch, size_t rowBytes, size_t rows, bool upload) {
    const size_t piece = rowBytes * rows, total = snnhip_tensor_bytes(t);
    if (piece * pieces.size() != total) return -1;
    if (planesAreDense(pieces.data(), pitch.data(), pieces.size(), rowBytes, rows))
        return (upload ? snnhip_tensor_upload_raw(t, pieces[0], total) : snnhip_tensor_download_raw(t, pieces[0], total)) == SNNHIP_OK ? 0 : -1;
    if (m->staging.size() < total) m->staging.resize(total);
    char* s = m->staging.data();
    if (!upload && snnhip_tensor_download_raw(t, s, total) != SNNHIP_OK) return -1;
    copyPlaneRows(s, pieces.data(), pitch.data(), pieces.size(), rowBytes, rows, upload);
    return upload ? (snnhip_tensor_upload_raw(t, s, total) == SNNHIP_OK ? 0 : -1) : 0;
}

// ... between the caller's planes and the luma tensor y and chroma tensor c of one end of the model (or the reference tensors of that extent)
static int movePlanesOf(snn_model* m, snnhip_tensor* y, snnhip_tensor* c, void* const* planes, const int* pitch, int n_planes, bool upload, bool planar) {
    if (!y || !c) return -1; // an RGB end, or no video frames at all
    if (n_planes != (planar ? 3 : 2)) return -1;
    int yd[4], cd[4];
    if (snnhip_tensor_dims(y, yd) != SNNHIP_OK || snnhip_tensor_dims(c, cd) != SNNHIP_OK || yd[0] != m->batch || yd[3] != 1) return -1;
    const size_t es = snnhip_tensor_dtype(y) == SNNHIP_U16 ? 2 : 1;
    const size_t yRow = static_cast<size_t>(yd[2]) * es, cRow = static_cast<size_t>(cd[2]) * static_cast<size_t>(cd[3]) * es;
    if (pitch[0] < 0 || static_cast<size_t>(pitch[0]) < yRow) return -1;
    for (int p = 1; p < n_planes; ++p)
        if (pitch[p] < 0 || static_cast<size_t>(pitch[p]) < cRow) return -1;
    for (int i = 0; i < m->batch * n_planes; ++i)
        if (!planes[i]) return -1;
    try {
        std::vector<size_t> lumaPitch, chromaPitch;
        std::vector<char*> luma, chroma; // in the order of the device tensors: [batch] and [batch] (CbCr) or [2 * batch] (Cb, Cr of each frame)
        for (int n = 0; n < m->batch; ++n) {
            luma.push_back(static_cast<char*>(planes[n * n_planes]));
            lumaPitch.push_back(static_cast<size_t>(pitch[0]));
            for (int p = 1; p < n_planes; ++p) {
                chroma.push_back(static_cast<char*>(planes[n * n_planes + p]));
                chromaPitch.push_back(static_cast<size_t>(pitch[p]));
            }
        }
        if (movePieces(m, y, luma, lumaPitch, yRow, static_cast<size_t>(yd[1]), upload) != 0) return -1;
        return movePieces(m, c, chroma, chromaPitch, cRow, static_cast<size_t>(cd[1]), upload);
    } catch (...) { // (std::bad_alloc of the staging buffer)
        return -2;
    }
}

static int moveFramePlanes(snn_model* m, void* const* planes, const int* pitch, int n_planes, bool upload) {
    if (!m || !planes || !pitch || !m->core) return -1;
    return movePlanesOf(m, upload ? m->core->frameInput() : m->core->frameOutput(), upload ? m->core->chromaInput() : m->core->chromaOutput(), planes, pitch, n_planes, upload,
                        upload ? m->core->planarVideo() : m->core->planarOutput());
}

int snn_model_upload_frame_planes(snn_model* m, const void* const* planes, const int* pitch_bytes, int n_planes) {
    return moveFramePlanes(m, const_cast<void* const*>(planes), pitch_bytes, n_planes, true);
}

int snn_model_download_frame_planes(snn_model* m, void* const* planes, const int* pitch_bytes, int n_planes) {
    return moveFramePlanes(m, planes, pitch_bytes, n_planes, false);
}

static void freeMetrics(snn_model::MetricsEnd& e) {
    if (e.plan) snnhip_plan_destroy(e.plan);
    if (e.ref) snnhip_tensor_free(e.ref);
    if (e.result) snnhip_tensor_free(e.result);
    e = snn_model::MetricsEnd();
}

int snn_model_destroy(snn_model* m) {
    if (!m) return 0;
    freeMetrics(m->metricsFrame); // (before the context goes: they live on its device)
    freeMetrics(m->metricsChroma);
    m->core.reset();
    m->inputs = ImageTextureArray(nullptr);
    m->outputs = ImageTextureArray(nullptr);
    delete m->context;
    delete m;
    return 0;
}

int snn_model_upload_frame_u8(snn_model* m, const unsigned char* nhwc) {
    snnhip_tensor* t = m && nhwc && !m->videoTensor ? m->core->frameInput() : nullptr; // (a video frame in front of an RGB model: _upload_frame_nv12 / _planes)
    if (t && snnhip_tensor_dtype(t) != SNNHIP_U8) return -1; // (a 16-bit end: snn_model_upload_frame_u16)
    return t && snnhip_tensor_upload_raw(t, nhwc, snnhip_tensor_bytes(t)) == SNNHIP_OK ? 0 : -1;
}

int snn_model_download_frame_u8(snn_model* m, unsigned char* nhwc) {
    snnhip_tensor* t = m && nhwc ? m->core->frameOutput() : nullptr;
    if (t && snnhip_tensor_dtype(t) != SNNHIP_U8) return -1;
    if (t && m->core->encodeOutput()) return -1; // (an NV12 frame: snn_model_download_frame_nv12)
    return t && snnhip_tensor_download_raw(t, nhwc, snnhip_tensor_bytes(t)) == SNNHIP_OK ? 0 : -1;
}

int snn_model_upload_frame_u16(snn_model* m, const unsigned short* nhwc) {
    snnhip_tensor* t = m && nhwc && !m->videoTensor ? m->core->frameInput() : nullptr;
    if (!t || snnhip_tensor_dtype(t) != SNNHIP_U16) return -1;
    return snnhip_tensor_upload_raw(t, nhwc, snnhip_tensor_bytes(t)) == SNNHIP_OK ? 0 : -1;
}

int snn_model_download_frame_u16(snn_model* m, unsigned short* nhwc) {
    snnhip_tensor* t = m && nhwc ? m->core->frameOutput() : nullptr;
    if (!t || snnhip_tensor_dtype(t) != SNNHIP_U16) return -1;
    if (m->core->frames().sink == FrameSpec::Sink::YUV420_FROM_TENSOR) return -1; // (a P010 / I010 frame of snn_model_create15: snn_model_download_frame_nv12 / _planes)
    return snnhip_tensor_download_raw(t, nhwc, snnhip_tensor_bytes(t)) == SNNHIP_OK ? 0 : -1;
}

// the reference tensor, the metrics plan and its result tensor for one output plane tensor `out`
static int makeMetricsEnd(snnhip_ctx* ctx, snnhip_tensor* out, int maxval, int shift, snn_model::MetricsEnd* e) {
    int d[4];
    if (snnhip_tensor_dims(out, d) != SNNHIP_OK) return -1;
    const int dtype = snnhip_tensor_dtype(out);
    snnhip_frame_metrics_desc desc{d[0], d[1], d[2], d[3], dtype, dtype == SNNHIP_U8 ? 255 : maxval, dtype == SNNHIP_U8 ? 0 : shift};
    if (snnhip_frame_metrics_plan_create(ctx, &desc, &e->plan) != SNNHIP_OK || snnhip_tensor_alloc(ctx, d[0], d[1], d[2], d[3], dtype, &e->ref) != SNNHIP_OK ||
        snnhip_tensor_alloc(ctx, d[0], 1, d[3], 2, SNNHIP_F32, &e->result) != SNNHIP_OK) {
        SNN_LOGE("snn_model_reference_frame: %s", snnhip_last_error());
        freeMetrics(*e);
        return -1;
    }
    e->maxval = desc.maxval;
    return 0;
}

// the first reference of a model allocates what its metrics need; false (logged) on a model whose output is a float tensor
static bool ensureMetrics(snn_model* m, const char* who) {
    snnhip_tensor* y = m->core->frameOutput();
    if (!y) {
        SNN_LOGE("%s: the model's output is a float tensor: frame metrics compare 8- / 16-bit output frames (create the model with an output frame format)", who);
        return false;
    }
    if (m->metricsFrame.plan) return true;
    snnhip_ctx* ctx = snn_model_hip_ctx(m);
    if (!ctx) return false;
    const FrameSpec& f = m->core->frames();
    // the depth of the output frame: the video end's for an RGB frame made from it, otherwise the model's own output map (the luma plane's on a video end)
    const bool fromVideo = f.sink == FrameSpec::Sink::RGB_FROM_YUV || f.sink == FrameSpec::Sink::RGB_FROM_YUV_FITTED;
    const bool encoded = f.sink == FrameSpec::Sink::YUV420_FROM_TENSOR; // both planes have the output stream's own depth
    const int lumaMaxval = encoded ? f.encMaxval : fromVideo ? f.maxval : f.model.out_maxval, lumaShift = encoded ? f.encShift : fromVideo ? f.shift : f.model.out_shift;
    if (makeMetricsEnd(ctx, y, lumaMaxval, lumaShift, &m->metricsFrame) != 0) return false;
    snnhip_tensor* c = m->core->chromaOutput();
    if (c && makeMetricsEnd(ctx, c, encoded ? f.encMaxval : f.maxval, encoded ? f.encShift : f.shift, &m->metricsChroma) != 0) {
        freeMetrics(m->metricsFrame);
        return false;
    }
    return true;
}

int snn_model_reference_frame(snn_model* m, const void* frame) {
    if (!m || !frame || !m->core) {
        SNN_LOGE("snn_model_reference_frame: null argument");
        return -1;
    }
    try {
        if (!ensureMetrics(m, "snn_model_reference_frame")) return -1;
        snnhip_tensor* y = m->metricsFrame.ref;
        snnhip_tensor* c = m->metricsChroma.ref;
        if (!c) return snnhip_tensor_upload_raw(y, frame, snnhip_tensor_bytes(y)) == SNNHIP_OK ? (m->referenceSet = true, 0) : -1;
        if (m->core->planarOutput()) {
            SNN_LOGE("snn_model_reference_frame: a planar output takes its reference through snn_model_reference_frame_planes, as it is downloaded");
            return -1;
        }
        // the layout of snn_model_download_frame_nv12: `batch` frames, each the luma plane followed by the interleaved chroma plane
        const size_t yb = snnhip_tensor_bytes(y) / static_cast<size_t>(m->batch), cb = snnhip_tensor_bytes(c) / static_cast<size_t>(m->batch);
        char* p = static_cast<char*>(const_cast<void*>(frame));
        if (movePlane(y, m->batch, p, yb + cb, 0, true) != 0 || movePlane(c, m->batch, p, yb + cb, yb, true) != 0) return -1;
        m->referenceSet = true;
        return 0;
    } catch (...) { // (std::bad_alloc of a staging buffer)
        return -2;
    }
}

int snn_model_reference_frame_planes(snn_model* m, const void* const* planes, const int* pitch_bytes, int n_planes) {
    if (!m || !planes || !pitch_bytes || !m->core) {
        SNN_LOGE("snn_model_reference_frame_planes: null argument");
        return -1;
    }
    try {
        if (!ensureMetrics(m, "snn_model_reference_frame_planes")) return -1;
        const int rc = movePlanesOf(m, m->metricsFrame.ref, m->metricsChroma.ref, const_cast<void* const*>(planes), pitch_bytes, n_planes, true, m->core->planarOutput());
        if (rc == 0) m->referenceSet = true;
        return rc;
    } catch (...) {
        return -2;
    }
}

int snn_model_frame_metrics(snn_model* m, snn_frame_metrics* rows, int max_rows) {
    if (!m || !rows || !m->core) {
        SNN_LOGE("snn_model_frame_metrics: null argument");
        return -1;
    }
    if (!m->referenceSet) {
        SNN_LOGE("snn_model_frame_metrics: no reference frame was set (snn_model_reference_frame / _frame_planes)");
        return -1;
    }
    try {
        const snn_model::MetricsEnd* ends[2] = {&m->metricsFrame, &m->metricsChroma};
        snnhip_tensor* outs[2] = {m->core->frameOutput(), m->core->chromaOutput()};
        std::vector<snnhip_frame_metrics_row> got[2];
        int dims[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        // both plans go onto the model's stream behind its last run, outside the recorded graph; the reads wait for them
        for (int e = 0; e < 2; ++e) {
            if (!ends[e]->plan) continue;
            const snnhip_tensor* in[2] = {outs[e], ends[e]->ref};
            if (!outs[e] || snnhip_plan_run_n(ends[e]->plan, in, 2, ends[e]->result) != SNNHIP_OK) {
                SNN_LOGE("snn_model_frame_metrics: %s", snnhip_last_error());
                return -1;
            }
        }
        for (int e = 0; e < 2; ++e) {
            if (!ends[e]->plan) continue;
            snnhip_tensor_dims(ends[e]->ref, dims[e]);
            got[e].resize(static_cast<size_t>(dims[e][0]) * dims[e][3]);
            if (snnhip_frame_metrics_read(ends[e]->plan, got[e].data(), static_cast<int>(got[e].size())) != static_cast<int>(got[e].size())) {
                SNN_LOGE("snn_model_frame_metrics: %s", snnhip_last_error());
                return -1;
            }
        }
        // image-major: the frame's (or luma plane's) channels, then the chroma plane's channels (interleaved: one plane, two channels; planar: plane
        // 2n is Cb and 2n + 1 Cr of image n, one channel each)
        const bool planar = m->core->planarOutput();
        int n = 0;
        auto put = [&](int image, int plane, int channel, const snnhip_frame_metrics_row& r, int maxval) {
            if (n < max_rows) rows[n] = snn_frame_metrics{image, plane, channel, r.sse, r.pixels, snnhip_frame_metrics_psnr(r.sse, r.pixels, maxval),
                                                          r.ssim_sum / static_cast<double>(r.windows)};
            ++n;
        };
        for (int image = 0; image < m->batch; ++image) {
            for (int c = 0; c < dims[0][3]; ++c) put(image, 0, c, got[0][static_cast<size_t>(image) * dims[0][3] + c], ends[0]->maxval);
            if (!ends[1]->plan) continue;
            if (planar)
                for (int p = 0; p < 2; ++p) put(image, 1 + p, 0, got[1][static_cast<size_t>(2 * image + p)], ends[1]->maxval);
            else
                for (int c = 0; c < dims[1][3]; ++c) put(image, 1, c, got[1][static_cast<size_t>(image) * dims[1][3] + c], ends[1]->maxval);
        }
        if (n > max_rows) {
            SNN_LOGE("snn_model_frame_metrics: room for %d rows, the model's output has %d", max_rows, n);
            return -1;
        }
        return n;
    } catch (...) {
        return -2;
    }
}

int snn_model_upload_input(snn_model* m, const float* nhwc) {
    if (m->videoTensor) return -1; // (frames go in: snn_model_upload_frame_nv12 / _planes)
    m->inputs[0].uploadNHWC(nhwc);
    return 0;
}

int snn_model_download_input(snn_model* m, float* nhwc) {
    if (!m || !nhwc) return -1;
    m->inputs[0].downloadNHWC(nhwc);
    return 0;
}

static int runModel(snn_model* m, bool deferSync) {
    try {
        MixedInferenceCore::RunParameters rp;
        rp.inputImages = &m->inputs;
        rp.outputImages = &m->outputs;
        rp.modelOutput.modelType = m->modelOutput.modelType;
        rp.deferSync = deferSync;
        m->core->run(rp);
        m->modelOutput = rp.modelOutput;
    } catch (const std::exception& e) {
        SNN_LOGE("snn_model_run: %s", e.what());
        return -2;
    } catch (...) {
        return -2;
    }
    return 0;
}

int snn_model_run(snn_model* m) { return runModel(m, false); }

int snn_model_run_async(snn_model* m) { return runModel(m, true); }

int snn_model_sync(snn_model* m) { return m->core->sync() ? 0 : -1; }

int snn_json_number(const char* text, double* out) {
    if (!text || !out) return -1;
    json::Value v;
    if (!json::parse(v, text).empty() || !v.isNumber()) return -1;
    *out = v.num;
    return 0;
}

int snn_model_set_type(snn_model* m, int model_type) {
    if (model_type < 0 || model_type > 3) return -1;
    m->modelOutput.modelType = static_cast<ModelType>(model_type);
    return 0;
}

int snn_model_classifier_output(snn_model* m) { return m->modelOutput.classifierOutput; }

static int copyRows(const std::vector<std::vector<float>>& rows, float* rows6, int max_rows) {
    int n = 0;
    for (auto& r : rows) {
        if (n >= max_rows) break;
        for (size_t k = 0; k < 6 && k < r.size(); ++k) rows6[n * 6 + static_cast<int>(k)] = r[k];
        ++n;
    }
    return n;
}

int snn_model_detections(snn_model* m, float* rows6, int max_rows) { return copyRows(m->modelOutput.detectionOutput, rows6, max_rows); }

int snn_yolo_decode(const float* head_coarse, const float* head_fine, int net_size, float* rows6, int max_rows) {
    return copyRows(dp::YOLOLayer::decode({head_coarse, head_fine}, net_size), rows6, max_rows);
}

int snn_model_upload_input_u8(snn_model* m, const unsigned char* pixels, int w, int h, int channels, const float means[4], const float norms[4],
                              const float resize_means[4], const float resize_norms[4]) {
    if (m->inC != 4 || m->videoTensor) return -1;
    auto arr = [](const float* p, float dflt) { return std::array<float, 4>{{p ? p[0] : dflt, p ? p[1] : dflt, p ? p[2] : dflt, p ? p[3] : dflt}}; };
    ImageTexture& t = m->inputs[0];
    t.loadU8AndNormalize(pixels, static_cast<uint32_t>(w), static_cast<uint32_t>(h), static_cast<uint32_t>(channels), arr(means, 0.0f), arr(norms, 1.0f));
    t.resize(static_cast<float>(w) / static_cast<float>(m->inW), static_cast<float>(h) / static_cast<float>(m->inH), arr(resize_means, 0.0f), arr(resize_norms, 1.0f));
    return (static_cast<int>(t.width()) == m->inW && static_cast<int>(t.height()) == m->inH) ? 0 : -2;
}

static ImageTexture& lastOutput(snn_model* m) { return m->core->stage(m->core->numStages() - 1).stageOutputs[0]; }

int snn_model_output_dims(snn_model* m, int hwc[3]) {
    ImageTexture& t = lastOutput(m);
    hwc[0] = static_cast<int>(t.height());
    hwc[1] = static_cast<int>(t.width());
    hwc[2] = static_cast<int>(t.channels());
    return 0;
}

int snn_model_batch(snn_model* m) { return m->batch; }

snnhip_ctx* snn_model_hip_ctx(snn_model* m) {
    auto* hc = dynamic_cast<HipContext*>(m->context);
    return hc ? hc->ctx : nullptr;
}

snnhip_tensor* snn_model_output_tensor(snn_model* m) { return lastOutput(m).tensor(); }

int snn_model_download_output(snn_model* m, float* nhwc) {
    if (m->core->frames().sink == FrameSpec::Sink::YUV420_FROM_TENSOR) return -1; // (the frame comes back: snn_model_download_frame_nv12 / _planes)
    lastOutput(m).downloadNHWC(nhwc);
    return 0;
}

int snn_model_num_stages(snn_model* m) { return static_cast<int>(m->core->numStages()); }

int snn_model_stage_info(snn_model* m, int stage, char* name, int name_len, int hwc[3], int* fused_away) {
    RenderStage& s = m->core->stage(static_cast<size_t>(stage));
    snprintf(name, static_cast<size_t>(name_len), "%s", s.layer->name.c_str());
    hwc[0] = static_cast<int>(s.layer->outputDesc.height);
    hwc[1] = static_cast<int>(s.layer->outputDesc.width);
    hwc[2] = static_cast<int>(s.layer->outputDesc.channels);
    *fused_away = (s.fusedAway ? 1 : 0) | (s.sideOfPrevious ? 2 : 0) | (s.groupWithPrevious ? 4 : 0);
    return 0;
}

int snn_model_download_stage(snn_model* m, int stage, float* nhwc) {
    RenderStage& s = m->core->stage(static_cast<size_t>(stage));
    if (s.layer->isInputLayer || s.stageOutputs.size() == 0 || !s.stageOutputs[0].isValid()) return -1;
    s.stageOutputs[0].downloadNHWC(nhwc);
    return 0;
}

int snn_model_describe(snn_model* m, char* buf, int buflen) {
    snprintf(buf, static_cast<size_t>(buflen), "%s", m->core->describe().c_str());
    return 0;
}

// the plan a stage really launches (nullptr: input layer, CPU stage, or folded into a later stage's fused plan)
static snnhip_plan* stagePlan(snn_model* m, int stage) {
    if (stage < 0 || stage >= static_cast<int>(m->core->numStages())) return nullptr;
    RenderStage& s = m->core->stage(static_cast<size_t>(stage));
    auto* ml = static_cast<dp::GenericModelLayer*>(s.layer->modelLayer);
    if (!ml || s.layer->isInputLayer || s.fusedAway || ml->getRenderPasses().size() != 1) return nullptr;
    auto* rp = dynamic_cast<dp::HipRenderPass*>(ml->getRenderPasses()[0].get());
    return (rp && !rp->skip) ? rp->plan : nullptr;
}

int snn_model_stage_plan_steps(snn_model* m, int stage) {
    snnhip_plan* p = stagePlan(m, stage);
    return p ? snnhip_plan_num_steps(p) : 0;
}

int snn_model_stage_plan_step(snn_model* m, int stage, int step, char* desc, int desc_len, double* flops, double* bytes) {
    snnhip_plan* p = stagePlan(m, stage);
    if (!p) return -1;
    if (desc && desc_len > 0 && snnhip_plan_step_describe(p, step, desc, static_cast<size_t>(desc_len)) != SNNHIP_OK) return -1;
    return snnhip_plan_step_cost(p, step, flops, bytes) == SNNHIP_OK ? 0 : -1;
}

int snn_model_profile_enable(snn_model* m, int enable) {
    m->core->suspendReplay(enable != 0); // a replayed hipGraph never calls the plans: profiled inferences run launch by launch
    for (int i = 0; i < static_cast<int>(m->core->numStages()); ++i)
        if (snnhip_plan* p = stagePlan(m, i))
            if (snnhip_plan_profile_enable(p, enable) != SNNHIP_OK) return -1;
    return 0;
}

int snn_model_suspend_replay(snn_model* m, int suspend) {
    m->core->suspendReplay(suspend != 0);
    return 0;
}

int snn_model_profile_read(snn_model* m, int stage, int step, double* total_ms, int* launches) {
    snnhip_plan* p = stagePlan(m, stage);
    if (!p) return -1;
    return snnhip_plan_profile_read(p, step, total_ms, launches) == SNNHIP_OK ? 0 : -1;
}

int snn_model_cost(snn_model* m, double* flops, double* bytes) {
    double f = 0, b = 0;
    for (int i = 0; i < static_cast<int>(m->core->numStages()); ++i)
        if (snnhip_plan* p = stagePlan(m, i)) {
            double pf = 0, pb = 0;
            if (snnhip_plan_cost(p, &pf, &pb) != SNNHIP_OK) return -1;
            f += pf;
            b += pb;
        }
    if (flops) *flops = f;
    if (bytes) *bytes = b;
    return 0;
}

int snn_model_time_stats(snn_model* m, char* names, int names_len, double* ms, int max_entries) {
    std::map<std::string, std::vector<double>> t;
    m->core->writeTimeStat(t);
    int n = 0;
    std::string all;
    for (auto& kv : t) {
        if (n >= max_entries) break;
        ms[n++] = kv.second.empty() ? 0.0 : kv.second.back();
        all += kv.first + "\n";
    }
    snprintf(names, static_cast<size_t>(names_len), "%s", all.c_str());
    return n;
}

int snn_conv_test_with_layer(int device, const float* input_hwc, const float* weights_oihw, const float* bias, int width, int height, int in_channels,
                             int out_channels, int kernel, int stride, int pad, int use_bn, const float* bn_gamma, const float* bn_mean,
                             const float* bn_var, const float* bn_beta, char* dump_path, int dump_path_len) {
    // ---- shaderUnitTest.cpp:192-230: hand-built InputLayer + Conv2D
    dp::InputLayerDesc inputDesc;
    inputDesc.inputHeight = static_cast<uint32_t>(width); // (sic) the reference swaps the two, shaderUnitTest.cpp:193-194
    inputDesc.inputWidth = static_cast<uint32_t>(height);
    inputDesc.inputChannels = static_cast<uint32_t>(in_channels);
    inputDesc.numInputPlanes = inputDesc.numOutputPlanes = static_cast<uint32_t>(in_channels);
    inputDesc.isInputLayer = true;
    auto inputLayer = std::make_shared<dp::InputLayerLayer>(inputDesc);
    inputLayer->setName("resnet18_cifar10_0223.json layer [00] InputLayerLayer");

    dp::Conv2DDesc desc;
    desc.isRange01 = false;
    desc.numOutputPlanes = static_cast<uint32_t>(out_channels);
    desc.numInputPlanes = static_cast<uint32_t>(in_channels);
    for (int p = 0; p < in_channels * out_channels; ++p) {
        WeightMat m(kernel, kernel);
        memcpy(m.data.data(), weights_oihw + static_cast<size_t>(p) * kernel * kernel, sizeof(float) * kernel * kernel);
        desc.weightsCvM.push_back(m);
    }
    for (int o = 0; o < out_channels; ++o) desc.biases.push_back(bias ? bias[o] : 0.0);
    desc.activation = "";
    desc.kernelSize = static_cast<uint32_t>(kernel);
    desc.stride = static_cast<uint32_t>(stride);
    desc.useBatchNormalization = use_bn != 0;
    if (use_bn) {
        desc.batchNormalization["gamma"].assign(bn_gamma, bn_gamma + out_channels);
        desc.batchNormalization["movingMean"].assign(bn_mean, bn_mean + out_channels);
        desc.batchNormalization["movingVariance"].assign(bn_var, bn_var + out_channels);
        desc.batchNormalization["beta"].assign(bn_beta, bn_beta + out_channels);
    }
    desc.useMultiInputs = false;
    desc.padding = "same";
    desc.paddingT = desc.paddingB = desc.paddingL = desc.paddingR = std::to_string(kernel / 2);
    desc.paddingMode = pad == 0 ? "constant" : pad == 1 ? "replicate" : "reflect";
    desc.weightMode = WeightAccessMethod::TEXTURES;
    std::shared_ptr<dp::GenericModelLayer> layer(dp::Conv2DCreator1(std::move(desc), false));
    layer->prevLayers.push_back(inputLayer);
    layer->setName("resnet18_cifar10_0223.json layer [01] Conv2D");
    inputLayer->nextLayers.push_back(layer);
    std::vector<std::shared_ptr<dp::GenericModelLayer>> layers{inputLayer, layer};

    // ---- :248-273: options, graph, textures, create, run
    snn_model m;
    m.context = createHipContext(device);
    m.inW = width;
    m.inH = height;
    m.inC = in_channels;
    dp::ShaderGenOptions sgo = makeOptions(width, height, in_channels, false);
    MixedInferenceCore::CreationParameters graph;
    static_cast<InferenceGraph&>(graph) = dp::generateInferenceGraph(layers, sgo);
    graph.dumpOutputs = true;
    makeIO(&m);
    m.inputs[0].uploadNHWC(input_hwc); // hwcToC4 + upload in the reference (:244-246, :265)
    m.core = MixedInferenceCore::create(m.context, graph);
    MixedInferenceCore::RunParameters rp;
    rp.inputImages = &m.inputs;
    rp.outputImages = &m.outputs;
    m.core->run(rp);
    snprintf(dump_path, static_cast<size_t>(dump_path_len), "%s/%s pass[0].dump", outputDir(), layer->getName().c_str()); // :275
    m.core.reset();
    m.inputs = ImageTextureArray(nullptr);
    m.outputs = ImageTextureArray(nullptr);
    layers.clear();
    layer.reset();
    inputLayer->nextLayers.clear();
    inputLayer.reset();
    delete m.context;
    return 0;
}

// A model the loader refuses (an exception of the parser or of a layer's validation) gives -2 and a one-line message in buf.
int snn_graph_summary(const char* json_path, int in_w, int in_h, int in_c, char* buf, int buflen) try {
    dp::ShaderGenOptions sgo = makeOptions(in_w, in_h, in_c, true);
    auto layers = dp::loadFromJsonModel(json_path, false, sgo.mrtMode, sgo.weightMode, false);
    InferenceGraph g = dp::generateInferenceGraph(layers, sgo);
    std::string out;
    for (size_t i = 0; i < g.layers.size(); ++i) {
        auto& l = *g.layers[i];
        std::string ins;
        for (auto& r : l.inputRefs) ins += (ins.empty() ? "" : ",") + std::to_string(r.index);
        out += formatString("%zu|%s|%d|%ux%ux%u|%s\n", i, l.name.c_str(), static_cast<int>(l.layerLoc), l.outputDesc.width, l.outputDesc.height,
                            l.outputDesc.channels, ins.c_str());
    }
    snprintf(buf, static_cast<size_t>(buflen), "%s", out.c_str());
    return static_cast<int>(g.layers.size());
} catch (const std::exception& e) {
    SNN_LOGE("snn_graph_summary: %s", e.what());
    if (buf && buflen > 0) snprintf(buf, static_cast<size_t>(buflen), "%s", e.what());
    return -2;
} catch (...) {
    if (buf && buflen > 0) buf[0] = 0;
    return -2;
}

int snn_dump_read(const char* path, int whdc[4], float* out, long out_floats) {
    RawImage img = RawImage::loadFromBIN(path);
    whdc[0] = static_cast<int>(img.width());
    whdc[1] = static_cast<int>(img.height());
    whdc[2] = static_cast<int>(img.depth());
    whdc[3] = static_cast<int>(img.channels());
    if (out) {
        const long n = static_cast<long>(img.size() / sizeof(float));
        if (n > out_floats) return -1;
        memcpy(out, img.data(), img.size());
    }
    return 0;
}

} // extern "C"
