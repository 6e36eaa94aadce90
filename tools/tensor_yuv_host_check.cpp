// tensor_yuv_host_check.cpp -- the host paths of the output-tensor -> video-frame feature that need no device, as a stand-alone program for a
// sanitizer build: the five coefficients with their refusals, every refusal of snn_model_create15 that returns before a
// model file is opened, and the resolved line against snn_model_create4's / snn_model_create5's / snn_model_create14's model parts (what needs a
// device is tests/test_frame_tensor_yuv_host_gpu.py's).  Built against lib/libsnn_core_asan.so by tools/sanitize.sh checks, as its siblings are.
// Exit status 0 and "tensor_yuv_host_check OK" when every expectation holds and the sanitizers stay silent.
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <utility>

#include "snn_c.h"
#include "snnhip.h"

static int failures = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            ++failures;                                                \
            fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
        }                                                              \
    } while (0)

static snn_video_tensor_io videoIn(int in_format = SNN_IO_NV12, int out_format = SNN_IO_FLOAT, int src_w = 64, int src_h = 48, int maxval = 255, int shift = 0) {
    return snn_video_tensor_io{in_format, out_format, src_w, src_h, maxval, shift, SNN_SITING_LEFT, SNN_RANGE_LIMITED, 0.299f, 0.114f, SNN_FILTER_LINEAR, {0, 0, 0, 0}, {1, 1, 1, 1},
                               1.0f,      {1, 1, 1, 1}, {0, 0, 0, 0}};
}

static snn_tensor_video_io io(int in_format = SNN_IO_FLOAT, int out_format = SNN_IO_NV12, int maxval = 255, int shift = 0, int siting = SNN_SITING_LEFT,
                              int range = SNN_RANGE_LIMITED, float kr = 0.299f, float kb = 0.114f) {
    snn_tensor_video_io v{in_format, out_format, maxval, shift, siting, range, kr, kb, {1, 1, 1, 1}, {0, 0, 0, 0}, {0, 0, 0, 0}, {1, 1, 1, 1}, videoIn()};
    if (in_format == SNN_IO_NV12 || in_format == SNN_IO_NV12_16 || in_format == SNN_IO_I420 || in_format == SNN_IO_I420_16)
        v.video_in = videoIn(in_format, SNN_IO_FLOAT, 64, 48, (in_format & 0x100) ? 1023 : 255, in_format == SNN_IO_NV12_16 ? 6 : 0);
    return v;
}

static int create15(const snn_tensor_video_io* v, int w = 16, int h = 12, int in_c = 3, int batch = 1) {
    snn_model* m = nullptr;
    const int rc = snn_model_create15("no/such/model.json", 0, w, h, in_c, 0, 1, 0, 0, 0, batch, v, &m);
    EXPECT(m == nullptr);
    char line[2048];
    EXPECT(snn_frames_resolve(15, v, w, h, in_c, batch, line, sizeof(line)) == -1); // the resolver and the entry point refuse the same requests
    return rc;
}

static std::string modelPart(int entry, const void* v, int in_c, std::string* rest = nullptr) {
    char line[2048] = "";
    EXPECT(snn_frames_resolve(entry, v, 16, 12, in_c, 1, line, sizeof(line)) == 0);
    const std::string s(line);
    const size_t bar = s.find(" | ");
    EXPECT(bar != std::string::npos);
    if (rest) *rest = bar == std::string::npos ? std::string() : s.substr(bar);
    return s.substr(0, bar);
}

int main() {
    // ---- the five coefficients against the formula in double, and as the reciprocals of yuv_rgb's
    for (int maxval : {255, 1023, 4095})
        for (int range : {int(SNNHIP_RANGE_LIMITED), int(SNNHIP_RANGE_FULL)})
            for (const std::pair<float, float>& m : {std::pair<float, float>{0.299f, 0.114f}, {0.2126f, 0.0722f}}) {
                float c[5] = {0, 0, 0, 0, 0}, y[7];
                EXPECT(snnhip_tensor_yuv_coefficients(maxval, range, m.first, m.second, c, 5) == SNNHIP_OK);
                EXPECT(snnhip_yuv_rgb_coefficients(maxval, range, m.first, m.second, y, 7) == SNNHIP_OK);
                const double k = (maxval + 1) / 256.0, yrange = range == SNNHIP_RANGE_LIMITED ? 219.0 * k : maxval, crange = range == SNNHIP_RANGE_LIMITED ? 224.0 * k : maxval;
                EXPECT(c[0] == static_cast<float>(range == SNNHIP_RANGE_LIMITED ? 16.0 * k : 0.0) && c[0] == y[0]);
                EXPECT(c[1] == static_cast<float>(yrange / maxval));
                EXPECT(c[2] == static_cast<float>(128.0 * k) && c[2] == y[1]);
                EXPECT(c[3] == static_cast<float>(crange / (2.0 * (1.0 - static_cast<double>(m.second)) * maxval)));
                EXPECT(c[4] == static_cast<float>(crange / (2.0 * (1.0 - static_cast<double>(m.first)) * maxval)));
                EXPECT(std::fabs(static_cast<double>(c[3]) * y[4] - 1.0) < 2e-7 && std::fabs(static_cast<double>(c[4]) * y[3] - 1.0) < 2e-7); // cbs cbu = crs crv = 1
                EXPECT(snnhip_tensor_yuv_coefficients(maxval, range, m.first, m.second, c, 4) == SNNHIP_E_INVALID); // the capacity refusal
            }
    {
        float c[5];
        EXPECT(snnhip_tensor_yuv_coefficients(255, 0, 0.299f, 0.114f, nullptr, 5) == SNNHIP_E_INVALID);
        EXPECT(snnhip_tensor_yuv_coefficients(255, 0, 0.299f, 0.114f, c, -1) == SNNHIP_E_INVALID);
        for (int maxval : {0, 127, 254, 256, 1000, 65536, -1}) EXPECT(snnhip_tensor_yuv_coefficients(maxval, 0, 0.299f, 0.114f, c, 5) == SNNHIP_E_INVALID);
        for (int range : {2, -1}) EXPECT(snnhip_tensor_yuv_coefficients(255, range, 0.299f, 0.114f, c, 5) == SNNHIP_E_INVALID);
        EXPECT(snnhip_tensor_yuv_coefficients(255, 0, 0.0f, 0.114f, c, 5) == SNNHIP_E_INVALID);
        EXPECT(snnhip_tensor_yuv_coefficients(255, 0, 0.299f, -0.1f, c, 5) == SNNHIP_E_INVALID);
        EXPECT(snnhip_tensor_yuv_coefficients(255, 0, 0.7f, 0.3f, c, 5) == SNNHIP_E_INVALID);
    }

    // ---- snn_model_create15: every refusal that returns before the model file is opened
    EXPECT(create15(nullptr) == -1);
    for (int f : {0, int(SNN_IO_R8), int(SNN_IO_RGB8), int(SNN_IO_RGBA8), int(SNN_IO_RGB16), 0x601, -1}) { // out_format: none of the four
        const snn_tensor_video_io v = io(SNN_IO_FLOAT, f);
        EXPECT(create15(&v) == -1);
    }
    for (int f : {int(SNN_IO_R16), int(SNN_IO_RGB16), int(SNN_IO_RGBA16), 0x601, 7, -1}) { // in_format: neither float, an 8-bit frame nor a video format
        const snn_tensor_video_io v = io(f);
        EXPECT(create15(&v) == -1);
    }
    {
        const snn_tensor_video_io rgb = io(SNN_IO_RGB8), rgba = io(SNN_IO_RGBA8), r8 = io(SNN_IO_R8);
        EXPECT(create15(&rgb, 16, 12, 4) == -1); // an 8-bit in_format of another channel count than the model input's
        EXPECT(create15(&rgba, 16, 12, 3) == -1);
        EXPECT(create15(&r8, 16, 12, 3) == -1);
    }
    {
        snn_tensor_video_io v = io(SNN_IO_NV12);
        v.video_in.out_format = SNN_IO_RGB8; // a video frame in front: its own output must be float
        EXPECT(create15(&v) == -1);
        v = io(SNN_IO_NV12);
        v.video_in.in_format = SNN_IO_I420; // ... and it repeats the in_format
        EXPECT(create15(&v) == -1);
        // everything snn_model_create14 refuses about video_in
        v = io(SNN_IO_NV12);
        EXPECT(create15(&v, 16, 12, 1) == -1 && create15(&v, 16, 12, 5) == -1); // in_c outside {3, 4}
        for (const std::pair<int, int>& s : {std::pair<int, int>{63, 48}, {64, 47}, {0, 48}, {64, -2}}) {
            v = io(SNN_IO_I420);
            v.video_in.src_w = s.first, v.video_in.src_h = s.second;
            EXPECT(create15(&v) == -1);
        }
        v = io(SNN_IO_NV12), v.video_in.filter = 2;
        EXPECT(create15(&v) == -1);
        v = io(SNN_IO_NV12), v.video_in.siting = 2;
        EXPECT(create15(&v) == -1);
        v = io(SNN_IO_NV12), v.video_in.range = -1;
        EXPECT(create15(&v) == -1);
        v = io(SNN_IO_NV12), v.video_in.maxval = 1023;
        EXPECT(create15(&v) == -1);
        v = io(SNN_IO_NV12_16), v.video_in.shift = 7;
        EXPECT(create15(&v) == -1);
        v = io(SNN_IO_NV12), v.video_in.kr = 0.0f;
        EXPECT(create15(&v) == -1);
    }
    const snn_tensor_video_io good = io();
    EXPECT(create15(&good, 0, 12) == -1);
    EXPECT(create15(&good, 16, 0) == -1);
    EXPECT(create15(&good, 16, 12, 3, 0) == -1); // batch below 1
    EXPECT(create15(&good, 16, 12, 3, -1) == -1);
    for (const snn_tensor_video_io& v :
         {io(0, SNN_IO_NV12, 255, 0, 2), io(0, SNN_IO_NV12, 255, 0, -1), io(0, SNN_IO_NV12, 255, 0, 1, 2), io(0, SNN_IO_NV12, 255, 0, 1, -1),         // siting, range
          io(0, SNN_IO_NV12, 256), io(0, SNN_IO_NV12, 127), io(0, SNN_IO_NV12, 1023), io(0, SNN_IO_NV12, 255, 1), io(0, SNN_IO_I420, 255, -1),         // maxval, shift
          io(0, SNN_IO_NV12_16, 65535), io(0, SNN_IO_NV12_16, 1023, 7), io(0, SNN_IO_I420_16, 1000), io(0, SNN_IO_I420_16, 8191), io(0, SNN_IO_I420_16, 1023, 16),
          io(0, SNN_IO_NV12, 255, 0, 1, 0, 0.0f), io(0, SNN_IO_I420, 255, 0, 1, 0, 0.299f, -0.1f), io(0, SNN_IO_NV12, 255, 0, 1, 0, 0.7f, 0.3f)})       // the matrix
        EXPECT(create15(&v) == -1);

    // ---- the resolved line: the model part is snn_model_create4's (snn_model_create5 with a null struct) ...
    for (int c : {1, 3, 4})
        for (int f : {int(SNN_IO_NV12), int(SNN_IO_NV12_16), int(SNN_IO_I420), int(SNN_IO_I420_16)}) {
            const snn_tensor_video_io v = io(SNN_IO_FLOAT, f, (f & 0x100) ? 1023 : 255, f == SNN_IO_NV12_16 ? 6 : 0);
            std::string rest;
            EXPECT(modelPart(15, &v, c, &rest) == modelPart(5, nullptr, c));
            EXPECT(rest.find("source=model sink=yuv420_from_tensor") != std::string::npos && rest.find("entry=snn_model_create15 | encode wide=") != std::string::npos);
            EXPECT(rest.find((f == SNN_IO_I420 || f == SNN_IO_I420_16) ? " planar=1 maxval=" : " planar=0 maxval=") != std::string::npos);
        }
    { // ... snn_model_create5's with the 8-bit input frame and a float output ...
        snn_tensor_video_io v = io(SNN_IO_RGB8);
        const float means[4] = {1, 2, 3, 4}, norms[4] = {0.5f, 0.25f, 0.125f, 1};
        for (int k = 0; k < 4; ++k) v.in_means[k] = means[k], v.in_norms[k] = norms[k];
        const snn_frame_io f{SNN_IO_RGB8, SNN_IO_FLOAT, {1, 2, 3, 4}, {0.5f, 0.25f, 0.125f, 1}, {1, 1, 1, 1}, {0, 0, 0, 0}};
        EXPECT(modelPart(15, &v, 3) == modelPart(5, &f, 3));
    }
    for (int f : {int(SNN_IO_NV12), int(SNN_IO_NV12_16), int(SNN_IO_I420), int(SNN_IO_I420_16)}) { // ... or snn_model_create14's, whose own line is kept whole
        const snn_tensor_video_io v = io(f, SNN_IO_I420);
        std::string rest15, rest14;
        EXPECT(modelPart(15, &v, 3, &rest15) == modelPart(14, &v.video_in, 3, &rest14));
        EXPECT(rest15.find("source=yuv420_tensor sink=yuv420_from_tensor") != std::string::npos && rest15.find(" | src=64x48 filter=1") != std::string::npos);
        EXPECT(rest14.find("encode") == std::string::npos && rest14.find("sink=model") != std::string::npos); // the earlier entry's line carries nothing of this one
    }

    if (failures) {
        fprintf(stderr, "tensor_yuv_host_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("tensor_yuv_host_check OK\n");
    return 0;
}
