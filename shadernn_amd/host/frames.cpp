// frames.cpp -- the public frame structs of include/snn_c.h resolved to one FrameSpec (snn/frames.h).  Each entry point's rules are its resolver;
// the checks they share are the functions at the top, and a struct that the header describes as "built exactly as" another one resolves THROUGH that
// one's resolver, so the statement holds by construction (tests/test_frame_paths.py and tools/frames_host_check.cpp compare the resolved lines).
#include "snn/frames.h"

#include <cstddef>
#include <cstring>

#include "snn/utils.h"

namespace snn {

using Source = FrameSpec::Source;
using Sink = FrameSpec::Sink;

// ---- the shared checks
static bool evenExtent(int w, int h) { return w >= 2 && h >= 2 && w % 2 == 0 && h % 2 == 0; } // 4:2:0: the chroma plane is half the extent
static bool knownSiting(int s) { return s == SNN_SITING_CENTRE || s == SNN_SITING_LEFT; }
static bool knownRange(int r) { return r == SNN_RANGE_LIMITED || r == SNN_RANGE_FULL; }
static bool knownMatrix(float kr, float kb) { return kr > 0.0f && kb > 0.0f && kr + kb < 1.0f; }
static bool isRgb8(int f) { return f == SNN_IO_RGB8 || f == SNN_IO_RGBA8; }
// maxval << shift fits the container: 2 bytes (shift 0..15), or 1 byte (shift 0)
static bool fitsContainer(int maxval, int shift, bool wide) {
    return maxval >= 1 && shift >= 0 && shift <= (wide ? 15 : 0) && (static_cast<long long>(maxval) << shift) <= (wide ? 65535 : 255);
}
// the depth whose luma maps follow from the range: k = (maxval + 1) / 256 is an integer
static bool rangedDepth(int maxval) { return maxval >= 255 && (maxval + 1) % 256 == 0; }
// a fitted 4:2:0 size: even, at least 2, and the chroma plane's ratio out / in within [1/2, 4]
static bool fittedSize(int ow, int oh, int w, int h) {
    return evenExtent(ow, oh) && w >= 1 && h >= 1 && 2ll * ow >= w && 2ll * oh >= h && ow <= 4ll * w && oh <= 4ll * h;
}

// the luma plane's maps of a video frame from its range (snn_model_create9 states them): k = (maxval + 1) / 256
static void lumaMapsOfRange(int maxval, int range, snn_video_io* video) {
    const double k = (maxval + 1) / 256.0;
    const double yoff = range == SNN_RANGE_LIMITED ? 16.0 * k : 0.0, yrange = range == SNN_RANGE_LIMITED ? 219.0 * k : maxval;
    video->in_mean = static_cast<float>(yoff);
    video->in_norm = static_cast<float>(1.0 / yrange);
    video->out_scale = static_cast<float>(yrange);
    video->out_offset = static_cast<float>(yoff);
}

// a luma-only model with R8 (R16 when wide) frames at both ends and one scalar map for all four channels.  An 8-bit output end is handed
// out_maxval = 65535 and shifts 0, as snn_model_create5 hands them: the same model
static void lumaModel(FrameSpec* s, bool wide, float mean, float norm, float scale, float offset, int maxval = 65535, int shift = 0) {
    s->model.in_format = s->model.out_format = wide ? int(SNN_IO_R16) : int(SNN_IO_R8);
    for (int c = 0; c < 4; ++c) {
        s->model.in_means[c] = mean;
        s->model.in_norms[c] = norm;
        s->model.out_scale[c] = scale;
        s->model.out_offset[c] = offset;
    }
    s->model.in_shift = s->model.out_shift = wide ? shift : 0;
    s->model.out_maxval = wide ? maxval : 65535;
}

ColorFormat frameColorFormat(int f) {
    switch (f) {
    case SNN_IO_R8: return ColorFormat::R8;
    case SNN_IO_RGB8: return ColorFormat::RGB8;
    case SNN_IO_RGBA8: return ColorFormat::RGBA8;
    case SNN_IO_R16: return ColorFormat::R16;
    case SNN_IO_RGB16: return ColorFormat::RGB16;
    case SNN_IO_RGBA16: return ColorFormat::RGBA16;
    default: return ColorFormat::NONE;
    }
}

int frameIoFormat(ColorFormat f) {
    for (int io : {int(SNN_IO_R8), int(SNN_IO_RGB8), int(SNN_IO_RGBA8), int(SNN_IO_R16), int(SNN_IO_RGB16), int(SNN_IO_RGBA16)})
        if (frameColorFormat(io) == f) return io;
    return SNN_IO_FLOAT;
}

static bool frameOrFloat(int f, bool allow16) { return f == SNN_IO_FLOAT || (frameColorFormat(f) != ColorFormat::NONE && (allow16 || !(f & 0x100))); }

// ---- snn_model_create6 (and, with the 8-bit formats only, snn_model_create5): the model's own ends, maps as given
bool resolveFrames(const snn_frame_io2* io, int, int, int in_c, int, FrameSpec* s) {
    s->entry = "snn_model_create6";
    if (!io) return true; // float at both ends
    if (!frameOrFloat(io->in_format, true) || !frameOrFloat(io->out_format, true)) return false;
    if (io->in_format != SNN_IO_FLOAT && (io->in_format & 0xff) != in_c) return false; // (low byte = channel count; the output's is known with the model)
    if ((io->in_format & 0x100) && (io->in_shift < 0 || io->in_shift > 15)) return false;
    if ((io->out_format & 0x100) && !fitsContainer(io->out_maxval, io->out_shift, true)) return false;
    s->model = *io;
    return true;
}

bool resolveFrames(const snn_frame_io* io, int in_w, int in_h, int in_c, int batch, FrameSpec* s) {
    snn_frame_io2 io2{};
    if (io) {
        if (!frameOrFloat(io->in_format, false) || !frameOrFloat(io->out_format, false)) return false; // (the 8-bit formats only)
        static_assert(offsetof(snn_frame_io2, in_shift) == sizeof(snn_frame_io) && offsetof(snn_frame_io2, out_offset) == offsetof(snn_frame_io, out_offset),
                      "snn_frame_io2 begins with snn_frame_io's fields");
        memcpy(&io2, io, sizeof(*io));
        io2.out_maxval = 65535;
    }
    const bool ok = resolveFrames(io ? &io2 : nullptr, in_w, in_h, in_c, batch, s);
    s->entry = "snn_model_create5";
    return ok;
}

// ---- snn_model_create7: RGB8 / RGBA8 at both ends, the luma plane through an R8 model
bool resolveFrames(const snn_colour_io* io, int, int, int in_c, int, FrameSpec* s) {
    if (!io || !isRgb8(io->format) || in_c != 1 || !knownMatrix(io->kr, io->kb)) return false;
    lumaModel(s, false, io->in_mean, io->in_norm, io->out_scale, io->out_offset);
    s->source = Source::RGB;
    s->sink = Sink::RGB_MERGED;
    s->channels = io->format & 0xff;
    s->kr = io->kr;
    s->kb = io->kb;
    s->entry = "snn_model_create7";
    return true;
}

// ---- snn_model_create8: NV12 / P010 at both ends, the luma plane through an R8 / R16 model, maps as given
bool resolveFrames(const snn_video_io* io, int in_w, int in_h, int in_c, int, FrameSpec* s) {
    if (!io || (io->format != SNN_IO_NV12 && io->format != SNN_IO_NV12_16) || in_c != 1) return false;
    const bool wide = io->format == SNN_IO_NV12_16;
    if (!evenExtent(in_w, in_h) || !knownSiting(io->siting)) return false;
    if (io->maxval > 4095 || !fitsContainer(io->maxval, io->shift, wide)) return false; // (P016 chroma is not built: include/snnhip.h)
    lumaModel(s, wide, io->in_mean, io->in_norm, io->out_scale, io->out_offset, io->maxval, io->shift);
    s->source = Source::YUV420;
    s->sink = Sink::CHROMA_UP;
    s->wide = wide;
    s->maxval = io->maxval;
    s->shift = io->shift;
    s->siting = io->siting;
    s->entry = "snn_model_create8";
    return true;
}

// ---- snn_model_create11: snn_model_create8's frames, the output resampled to out_w x out_h
bool resolveFrames(const snn_fit_io* io, int in_w, int in_h, int in_c, int batch, FrameSpec* s) {
    if (!io || !fittedSize(io->out_w, io->out_h, in_w, in_h) || !resolveFrames(&io->video, in_w, in_h, in_c, batch, s)) return false;
    s->sink = Sink::FITTED;
    s->fitW = io->out_w;
    s->fitH = io->out_h;
    s->entry = "snn_model_create11";
    return true;
}

// ---- snn_model_create9: snn_model_create8's frames in with the range's maps, RGB out
bool resolveFrames(const snn_video_rgb_io* io, int in_w, int in_h, int in_c, int batch, FrameSpec* s) {
    if (!io || (io->in_format != SNN_IO_NV12 && io->in_format != SNN_IO_NV12_16)) return false;
    const bool wide = io->in_format == SNN_IO_NV12_16;
    if (wide ? (io->out_format != SNN_IO_RGB16 && io->out_format != SNN_IO_RGBA16) : !isRgb8(io->out_format)) return false;
    if (!knownRange(io->range) || !rangedDepth(io->maxval) || !knownMatrix(io->kr, io->kb)) return false;
    snn_video_io video{io->in_format, io->maxval, io->shift, io->siting, 0, 0, 0, 0};
    lumaMapsOfRange(io->maxval, io->range, &video);
    if (!resolveFrames(&video, in_w, in_h, in_c, batch, s)) return false;
    s->sink = Sink::RGB_FROM_YUV;
    s->channels = io->out_format & 0xff;
    s->range = io->range;
    s->kr = io->kr;
    s->kb = io->kb;
    s->entry = "snn_model_create9";
    return true;
}

// ---- snn_model_create10: RGB8 / RGBA8 in, NV12 out; full-range luma in (rgb_luma), the range's luma codes out.  The extent may be odd: only
// r * extent must be even, which framesFitModel decides once the model file gives r
bool resolveFrames(const snn_encode_io* io, int, int, int in_c, int, FrameSpec* s) {
    if (!io || !isRgb8(io->in_format) || io->out_format != SNN_IO_NV12 || in_c != 1) return false;
    if (!knownSiting(io->siting) || !knownRange(io->range) || !knownMatrix(io->kr, io->kb)) return false;
    const bool limited = io->range == SNN_RANGE_LIMITED;
    lumaModel(s, false, 0.0f, 1.0f / 255.0f, limited ? 219.0f : 255.0f, limited ? 16.0f : 0.0f);
    s->source = Source::RGB;
    s->sink = Sink::YUV420_FROM_RGB;
    s->channels = io->in_format & 0xff;
    s->siting = io->siting;
    s->range = io->range;
    s->kr = io->kr;
    s->kb = io->kb;
    s->entry = "snn_model_create10";
    return true;
}

// ---- snn_model_create12: each path is its NV12 counterpart's with separate Cb and Cr planes
bool resolveFrames(const snn_planar_io* io, int in_w, int in_h, int in_c, int batch, FrameSpec* s) {
    if (!io) return false;
    const bool fitted = io->out_w != 0 || io->out_h != 0, wide = io->in_format == SNN_IO_I420_16;
    const int interleaved = wide ? SNN_IO_NV12_16 : SNN_IO_NV12;
    bool ok = false;
    if (isRgb8(io->in_format)) { // capture in, planar out: snn_model_create10's path
        const snn_encode_io e{io->in_format, SNN_IO_NV12, io->siting, io->range, io->kr, io->kb};
        ok = io->out_format == SNN_IO_I420 && !fitted && resolveFrames(&e, in_w, in_h, in_c, batch, s);
    } else if (io->in_format != SNN_IO_I420 && !wide) {
        return false;
    } else if (io->out_format != io->in_format) { // planar in, RGB out: snn_model_create9's path, which pairs the formats (RGB at a fitted size is not built)
        const snn_video_rgb_io v{interleaved, io->out_format, io->maxval, io->shift, io->siting, io->range, io->kr, io->kb};
        ok = !fitted && resolveFrames(&v, in_w, in_h, in_c, batch, s);
    } else { // planar in, planar out: snn_model_create8's path, or snn_model_create11's with a fitted size.  The luma maps follow from the range, which
             // needs snn_model_create9's depth rule (the matrix is not used: kr and kb are not looked at)
        if (!knownRange(io->range) || !rangedDepth(io->maxval)) return false;
        snn_fit_io f{{interleaved, io->maxval, io->shift, io->siting, 0, 0, 0, 0}, io->out_w, io->out_h};
        lumaMapsOfRange(io->maxval, io->range, &f.video);
        ok = fitted ? resolveFrames(&f, in_w, in_h, in_c, batch, s) : resolveFrames(&f.video, in_w, in_h, in_c, batch, s);
    }
    s->planar = true;
    s->entry = "snn_model_create12";
    return ok;
}

// ---- snn_model_create13: RGB at out_w x out_h.  A video source resolves through snn_model_create9's struct (snn_model_create12's for planar planes),
// a colour source through snn_model_create7's with the full-range luma maps; only the sink and the size are added.  The ratio rules that need no r:
// the r-fold frame (r = 1..4) is brought down by at most a half, so out / in lies in [1/2, 4]; a colour frame is never shrunk, [1, 4]
bool resolveFrames(const snn_rgb_fit_io* io, int in_w, int in_h, int in_c, int batch, FrameSpec* s) {
    if (!io || io->out_w < 1 || io->out_h < 1 || in_w < 1 || in_h < 1) return false;
    if (io->out_w > 4ll * in_w || io->out_h > 4ll * in_h) return false;
    if (isRgb8(io->in_format)) {
        if (io->out_format != io->in_format || io->out_w < in_w || io->out_h < in_h) return false;
        const snn_colour_io c{io->in_format, io->kr, io->kb, 0.0f, 1.0f / 255.0f, 255.0f, 0.0f};
        if (!resolveFrames(&c, in_w, in_h, in_c, batch, s)) return false;
        s->sink = Sink::RGB_MERGED_FITTED;
    } else {
        if (2ll * io->out_w < in_w || 2ll * io->out_h < in_h) return false;
        const bool planar = io->in_format == SNN_IO_I420 || io->in_format == SNN_IO_I420_16;
        if (!isRgb8(io->out_format) && io->out_format != SNN_IO_RGB16 && io->out_format != SNN_IO_RGBA16) return false; // (the resolvers below pair it with the input)
        if (planar) {
            const snn_planar_io p{io->in_format, io->out_format, io->maxval, io->shift, io->siting, io->range, io->kr, io->kb, 0, 0};
            if (!resolveFrames(&p, in_w, in_h, in_c, batch, s)) return false;
        } else {
            const snn_video_rgb_io v{io->in_format, io->out_format, io->maxval, io->shift, io->siting, io->range, io->kr, io->kb};
            if (!resolveFrames(&v, in_w, in_h, in_c, batch, s)) return false;
        }
        if (s->sink != Sink::RGB_FROM_YUV) return false;
        s->sink = Sink::RGB_FROM_YUV_FITTED;
    }
    s->fitW = io->out_w;
    s->fitH = io->out_h;
    s->entry = "snn_model_create13";
    return true;
}

// ---- snn_model_create14: a 4:2:0 frame of src_w x src_h in front of an RGB(A) model.  The model resolves as snn_model_create4's (float at both
// ends), or through snn_model_create5's struct with a float input and the 8-bit out_format
bool resolveFrames(const snn_video_tensor_io* io, int in_w, int in_h, int in_c, int batch, FrameSpec* s) {
    if (!io || (in_c != 3 && in_c != 4)) return false;
    const bool planar = io->in_format == SNN_IO_I420 || io->in_format == SNN_IO_I420_16, wide = io->in_format == SNN_IO_NV12_16 || io->in_format == SNN_IO_I420_16;
    if (!planar && io->in_format != SNN_IO_NV12 && io->in_format != SNN_IO_NV12_16) return false;
    if (!evenExtent(io->src_w, io->src_h) || (io->filter != SNN_FILTER_NEAREST && io->filter != SNN_FILTER_LINEAR)) return false;
    if (!knownSiting(io->siting) || !knownRange(io->range) || !rangedDepth(io->maxval) || !knownMatrix(io->kr, io->kb)) return false;
    if (io->maxval > 4095 || !fitsContainer(io->maxval, io->shift, wide)) return false; // (as snn_model_create8)
    if (io->out_format == SNN_IO_FLOAT) {
        if (!resolveFrames(static_cast<const snn_frame_io*>(nullptr), in_w, in_h, in_c, batch, s)) return false;
    } else {
        snn_frame_io f{SNN_IO_FLOAT, io->out_format, {0, 0, 0, 0}, {1, 1, 1, 1}, {0, 0, 0, 0}, {0, 0, 0, 0}};
        memcpy(f.out_scale, io->out_scale, sizeof(f.out_scale));
        memcpy(f.out_offset, io->out_offset, sizeof(f.out_offset));
        if (!resolveFrames(&f, in_w, in_h, in_c, batch, s)) return false;
    }
    s->source = Source::YUV420_TENSOR;
    s->channels = in_c;
    s->wide = wide;
    s->maxval = io->maxval;
    s->shift = io->shift;
    s->siting = io->siting;
    s->range = io->range;
    s->kr = io->kr;
    s->kb = io->kb;
    s->planar = planar;
    s->srcW = io->src_w;
    s->srcH = io->src_h;
    s->filter = io->filter;
    for (int c = 0; c < 3; ++c) s->tensorMeans[c] = io->means[c], s->tensorNorms[c] = io->norms[c];
    s->alpha = io->alpha;
    s->entry = "snn_model_create14";
    return true;
}

// ---- snn_model_create15: the output tensor of an RGB(A) model to a 4:2:0 frame.  The model resolves as snn_model_create4's, through
// snn_model_create5's struct with the 8-bit in_format and a float output, or through snn_model_create14's struct with a float output; only the sink
// and the output stream are added
bool resolveFrames(const snn_tensor_video_io* io, int in_w, int in_h, int in_c, int batch, FrameSpec* s) {
    if (!io) return false;
    auto video = [](int f) { return f == SNN_IO_NV12 || f == SNN_IO_NV12_16 || f == SNN_IO_I420 || f == SNN_IO_I420_16; };
    if (!video(io->out_format)) return false;
    const bool planar = io->out_format == SNN_IO_I420 || io->out_format == SNN_IO_I420_16, wide = io->out_format == SNN_IO_NV12_16 || io->out_format == SNN_IO_I420_16;
    if (!knownSiting(io->siting) || !knownRange(io->range) || !rangedDepth(io->maxval) || !knownMatrix(io->kr, io->kb)) return false;
    if (io->maxval > 4095 || !fitsContainer(io->maxval, io->shift, wide)) return false; // (as snn_model_create8)
    if (io->in_format == SNN_IO_FLOAT) {
        if (!resolveFrames(static_cast<const snn_frame_io*>(nullptr), in_w, in_h, in_c, batch, s)) return false;
    } else if (video(io->in_format)) {
        if (io->video_in.in_format != io->in_format || io->video_in.out_format != SNN_IO_FLOAT || !resolveFrames(&io->video_in, in_w, in_h, in_c, batch, s)) return false;
    } else {
        if (!frameOrFloat(io->in_format, false)) return false; // (the 8-bit formats only)
        snn_frame_io f{io->in_format, SNN_IO_FLOAT, {0, 0, 0, 0}, {1, 1, 1, 1}, {1, 1, 1, 1}, {0, 0, 0, 0}};
        memcpy(f.in_means, io->in_means, sizeof(f.in_means));
        memcpy(f.in_norms, io->in_norms, sizeof(f.in_norms));
        if (!resolveFrames(&f, in_w, in_h, in_c, batch, s)) return false;
    }
    s->sink = Sink::YUV420_FROM_TENSOR;
    s->encWide = wide;
    s->encPlanar = planar;
    s->encMaxval = io->maxval;
    s->encShift = io->shift;
    s->encSiting = io->siting;
    s->encRange = io->range;
    s->encKr = io->kr;
    s->encKb = io->kb;
    for (int c = 0; c < 3; ++c) s->encScale[c] = io->out_scale[c], s->encOffset[c] = io->out_offset[c];
    s->entry = "snn_model_create15";
    return true;
}

bool resolveFrames(int entry, const void* io, int in_w, int in_h, int in_c, int batch, FrameSpec* s) {
    if (!s || batch < 1 || in_w < 1 || in_h < 1 || in_c < 1) return false;
    *s = FrameSpec();
    switch (entry) {
    case 5: return resolveFrames(static_cast<const snn_frame_io*>(io), in_w, in_h, in_c, batch, s);
    case 6: return resolveFrames(static_cast<const snn_frame_io2*>(io), in_w, in_h, in_c, batch, s);
    case 7: return resolveFrames(static_cast<const snn_colour_io*>(io), in_w, in_h, in_c, batch, s);
    case 8: return resolveFrames(static_cast<const snn_video_io*>(io), in_w, in_h, in_c, batch, s);
    case 9: return resolveFrames(static_cast<const snn_video_rgb_io*>(io), in_w, in_h, in_c, batch, s);
    case 10: return resolveFrames(static_cast<const snn_encode_io*>(io), in_w, in_h, in_c, batch, s);
    case 11: return resolveFrames(static_cast<const snn_fit_io*>(io), in_w, in_h, in_c, batch, s);
    case 12: return resolveFrames(static_cast<const snn_planar_io*>(io), in_w, in_h, in_c, batch, s);
    case 13: return resolveFrames(static_cast<const snn_rgb_fit_io*>(io), in_w, in_h, in_c, batch, s);
    case 14: return resolveFrames(static_cast<const snn_video_tensor_io*>(io), in_w, in_h, in_c, batch, s);
    case 15: return resolveFrames(static_cast<const snn_tensor_video_io*>(io), in_w, in_h, in_c, batch, s);
    default: return false;
    }
}

bool framesFitModel(const FrameSpec& spec, int in_w, int in_h, const InferenceGraph::IODesc& out) {
    if (spec.source == Source::MODEL && spec.sink == Sink::MODEL) return true;
    if (spec.sink == Sink::YUV420_FROM_TENSOR) { // any model of 3 or 4 output channels and an even output extent: the frame starts in its output tensor
        if ((out.channels == 3 || out.channels == 4) && evenExtent(static_cast<int>(out.width), static_cast<int>(out.height))) return true;
        SNN_LOGE("%s: a 4:2:0 output frame needs a model of 3 or 4 output channels and an even output extent; this one gives %ux%ux%u", spec.entry, out.height, out.width,
                 out.channels);
        return false;
    }
    if (spec.source == Source::YUV420_TENSOR) return true; // any model of 3 or 4 input channels: the frame ends in its input tensor
    // the model must be luma-only: one channel out, at 1..4 times the input's extent
    const uint32_t w = static_cast<uint32_t>(in_w), h = static_cast<uint32_t>(in_h), r = out.width / w;
    if (out.channels != 1 || r < 1 || r > 4 || out.width != r * w || out.height != r * h) return false;
    // a 4:2:0 frame made from RGB: r = 2..4 (r = 1 would decimate the chroma grid) and an even extent
    if (spec.sink == Sink::YUV420_FROM_RGB && (r < 2 || (r * w) % 2 || (r * h) % 2)) return false;
    if (spec.sink != Sink::FITTED && spec.sink != Sink::RGB_FROM_YUV_FITTED && spec.sink != Sink::RGB_MERGED_FITTED) return true;
    // the r-fold frame is resampled DOWN to the target: r * in / 2 <= out <= r * in on both axes; and a colour frame that went in is never shrunk
    // (its chroma differences are only enlarged), so r = 1 then permits out = in alone
    const bool colourIn = spec.sink == Sink::RGB_MERGED_FITTED;
    const long long rw = static_cast<long long>(r) * in_w, rh = static_cast<long long>(r) * in_h;
    auto fitsAt = [&](long long q) {
        return spec.fitW <= q * in_w && spec.fitH <= q * in_h && 2ll * spec.fitW >= q * in_w && 2ll * spec.fitH >= q * in_h && (!colourIn || (spec.fitW >= in_w && spec.fitH >= in_h));
    };
    if (fitsAt(r)) return true;
    std::string fits;
    for (int q = 1; q <= 4; ++q)
        if (fitsAt(q)) fits += (fits.empty() ? "" : ", ") + std::to_string(q);
    const char* why = (spec.fitW > rw || spec.fitH > rh)             ? "larger than that"
                      : (2ll * spec.fitW < rw || 2ll * spec.fitH < rh) ? "less than half of that"
                                                                       : "smaller than the colour frame that goes in, which is never shrunk";
    SNN_LOGE("%s: the model is r = %u: %dx%d -> %lldx%lld, and %dx%d is %s; %s%s", spec.entry, r, in_w, in_h, rw, rh, spec.fitW, spec.fitH, why,
             fits.empty() ? "no r = 1..4 fits both axes" : "a model of r = ", fits.c_str());
    return false;
}

std::string formatFrameSpec(const FrameSpec& s) {
    static const char* const sources[] = {"model", "rgb", "yuv420", "yuv420_tensor"};
    static const char* const sinks[] = {"model", "rgb_merged", "chroma_up", "fitted", "rgb_from_yuv", "yuv420_from_rgb", "rgb_from_yuv_fitted", "rgb_merged_fitted",
                                        "yuv420_from_tensor"};
    static_assert(sizeof(sources) / sizeof(*sources) == static_cast<size_t>(Source::YUV420_TENSOR) + 1, "one name for every FrameSpec::Source");
    static_assert(sizeof(sinks) / sizeof(*sinks) == static_cast<size_t>(Sink::YUV420_FROM_TENSOR) + 1, "one name for every FrameSpec::Sink");
    const snn_frame_io2& m = s.model;
    auto four = [](const float* v) { return formatString("%.9g,%.9g,%.9g,%.9g", v[0], v[1], v[2], v[3]); };
    // (the lines of snn_model_create5..13 stay as they were: what only snn_model_create14 sets is appended to its own line alone)
    const std::string tensor = s.source != Source::YUV420_TENSOR
                                   ? std::string()
                                   : formatString(" | src=%dx%d filter=%d tensor_means=%.9g,%.9g,%.9g tensor_norms=%.9g,%.9g,%.9g alpha=%.9g", s.srcW, s.srcH, s.filter, s.tensorMeans[0],
                                                  s.tensorMeans[1], s.tensorMeans[2], s.tensorNorms[0], s.tensorNorms[1], s.tensorNorms[2], s.alpha);
    // ... and what only snn_model_create15 sets to its own line alone
    const std::string encode = s.sink != Sink::YUV420_FROM_TENSOR
                                   ? std::string()
                                   : formatString(" | encode wide=%d planar=%d maxval=%d shift=%d siting=%d range=%d kr=%.9g kb=%.9g enc_scale=%.9g,%.9g,%.9g enc_offset=%.9g,%.9g,%.9g",
                                                  s.encWide ? 1 : 0, s.encPlanar ? 1 : 0, s.encMaxval, s.encShift, s.encSiting, s.encRange, s.encKr, s.encKb, s.encScale[0], s.encScale[1],
                                                  s.encScale[2], s.encOffset[0], s.encOffset[1], s.encOffset[2]);
    return formatString("in=0x%x out=0x%x means=%s norms=%s scale=%s offset=%s in_shift=%d out_maxval=%d out_shift=%d", m.in_format, m.out_format, four(m.in_means).c_str(),
                        four(m.in_norms).c_str(), four(m.out_scale).c_str(), four(m.out_offset).c_str(), m.in_shift, m.out_maxval, m.out_shift) +
           formatString(" | source=%s sink=%s channels=%d wide=%d maxval=%d shift=%d siting=%d range=%d kr=%.9g kb=%.9g fit=%dx%d planar=%d | entry=%s",
                        sources[static_cast<int>(s.source)], sinks[static_cast<int>(s.sink)], s.channels, s.wide ? 1 : 0, s.maxval, s.shift, s.siting, s.range, s.kr, s.kb,
                        s.fitW, s.fitH, s.planar ? 1 : 0, s.entry) +
           tensor + encode;
}

} // namespace snn
