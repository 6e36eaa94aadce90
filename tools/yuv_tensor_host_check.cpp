// yuv_tensor_host_check.cpp -- the host paths of the video-frame -> input-tensor feature that need no device, as a stand-alone program for a sanitizer
// build: the sampling table of one axis with its refusals, every refusal of snn_model_create14 that returns before a model
// file is opened, and the resolved line against snn_model_create4's / snn_model_create5's (what needs a device is
// tests/test_frame_yuv_tensor_host_gpu.py's).  Built against lib/libsnn_core_asan.so by tools/sanitize.sh checks, as its siblings are.
// Exit status 0 and "yuv_tensor_host_check OK" when every expectation holds and the sanitizers stay silent.
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

static snn_video_tensor_io io(int in_format = SNN_IO_NV12, int out_format = SNN_IO_FLOAT, int src_w = 64, int src_h = 48, int maxval = 255, int shift = 0,
                              int siting = SNN_SITING_LEFT, int range = SNN_RANGE_LIMITED, float kr = 0.299f, float kb = 0.114f, int filter = SNN_FILTER_LINEAR) {
    return snn_video_tensor_io{in_format, out_format, src_w, src_h, maxval, shift, siting, range, kr, kb, filter, {0, 0, 0, 0}, {1, 1, 1, 1}, 1.0f, {255, 255, 255, 255}, {0, 0, 0, 0}};
}

static int create14(const snn_video_tensor_io* v, int w = 16, int h = 12, int in_c = 3, int batch = 1) {
    snn_model* m = nullptr;
    const int rc = snn_model_create14("no/such/model.json", 0, w, h, in_c, 0, 1, 0, 0, 0, batch, v, &m);
    EXPECT(m == nullptr);
    char line[1024];
    EXPECT(snn_frames_resolve(14, v, w, h, in_c, batch, line, sizeof(line)) == -1); // the resolver and the entry point refuse the same requests
    return rc;
}

static std::string modelPart(int entry, const void* v, int in_c, std::string* rest = nullptr) {
    char line[1024] = "";
    EXPECT(snn_frames_resolve(entry, v, 16, 12, in_c, 1, line, sizeof(line)) == 0);
    const std::string s(line);
    const size_t bar = s.find(" | ");
    EXPECT(bar != std::string::npos);
    if (rest) *rest = bar == std::string::npos ? std::string() : s.substr(bar);
    return s.substr(0, bar);
}

int main() {
    // the table of one axis: [out] weights and [out][2] indices, written into buffers of exactly that size
    for (int filter : {SNNHIP_YUV_TENSOR_NEAREST, SNNHIP_YUV_TENSOR_LINEAR})
        for (const std::pair<int, int>& p : {std::pair<int, int>{1, 1}, {2, 1}, {2, 5}, {64, 7}, {8, 8}, {7, 19}, {1080, 224}, {1920, 416}, {720, 720}, {3, 1}, {1, 9}}) {
            const int I = p.first, O = p.second;
            float* a = new float[O];
            int* idx = new int[2 * O];
            EXPECT(snnhip_yuv_tensor_taps(I, O, filter, a, idx, O) == SNNHIP_OK);
            for (int o = 0; o < O; ++o) {
                EXPECT(idx[2 * o] >= 0 && idx[2 * o] <= idx[2 * o + 1] && idx[2 * o + 1] <= idx[2 * o] + 1 && idx[2 * o + 1] < I);
                EXPECT(a[o] >= 0.0f && a[o] < 1.0f);
                if (filter == SNNHIP_YUV_TENSOR_NEAREST) {
                    EXPECT(a[o] == 0.0f && idx[2 * o] == idx[2 * o + 1] && idx[2 * o] == static_cast<int>(((2ll * o + 1) * I) / (2ll * O)));
                } else { // u = num / den exactly; i0 = floor(u), the fraction rounded to double, then to float
                    const long long num = (2ll * o + 1) * I - O, den = 2ll * O;
                    long long i0 = num / den;
                    if (num < 0 && i0 * den != num) --i0;
                    EXPECT(a[o] == static_cast<float>(static_cast<double>(num - i0 * den) / static_cast<double>(den)));
                    EXPECT(idx[2 * o] == static_cast<int>(i0 < 0 ? 0 : i0 > I - 1 ? I - 1 : i0));
                    if (I == O) EXPECT(a[o] == 0.0f && idx[2 * o] == o); // ratio 1: every output pixel is its own source pixel
                }
            }
            EXPECT(snnhip_yuv_tensor_taps(I, O, filter, a, idx, O - 1) == SNNHIP_E_INVALID); // the capacity refusal: nothing is written past it
            delete[] a;
            delete[] idx;
        }
    {
        float a[8];
        int idx[16];
        EXPECT(snnhip_yuv_tensor_taps(0, 4, 1, a, idx, 8) == SNNHIP_E_INVALID);
        EXPECT(snnhip_yuv_tensor_taps(4, 0, 1, a, idx, 8) == SNNHIP_E_INVALID);
        EXPECT(snnhip_yuv_tensor_taps(-4, -4, 1, a, idx, 8) == SNNHIP_E_INVALID);
        EXPECT(snnhip_yuv_tensor_taps((1 << 30) + 1, 4, 1, a, idx, 8) == SNNHIP_E_INVALID);
        EXPECT(snnhip_yuv_tensor_taps(4, 4, 2, a, idx, 8) == SNNHIP_E_INVALID);
        EXPECT(snnhip_yuv_tensor_taps(4, 4, -1, a, idx, 8) == SNNHIP_E_INVALID);
        EXPECT(snnhip_yuv_tensor_taps(4, 4, 1, nullptr, idx, 8) == SNNHIP_E_INVALID);
        EXPECT(snnhip_yuv_tensor_taps(4, 4, 1, a, nullptr, 8) == SNNHIP_E_INVALID);
        EXPECT(snnhip_yuv_tensor_taps(4, 8, 1, a, idx, 7) == SNNHIP_E_INVALID);
        EXPECT(snnhip_yuv_tensor_taps(4, 8, 1, a, idx, -1) == SNNHIP_E_INVALID);
        EXPECT(snnhip_yuv_tensor_taps(4, 8, 1, a, idx, 8) == SNNHIP_OK); // exactly enough room
    }

    // ---- snn_model_create14: every refusal that returns before the model file is opened
    EXPECT(create14(nullptr) == -1);
    for (int f : {0, int(SNN_IO_R8), int(SNN_IO_RGB8), int(SNN_IO_RGBA8), int(SNN_IO_RGB16), 0x601, -1}) { // unknown input formats
        const snn_video_tensor_io v = io(f);
        EXPECT(create14(&v) == -1);
    }
    for (int f : {int(SNN_IO_NV12), int(SNN_IO_I420), int(SNN_IO_RGB16), int(SNN_IO_RGBA16), int(SNN_IO_R16), 7, -1}) { // neither float nor an 8-bit frame
        const snn_video_tensor_io v = io(SNN_IO_NV12, f);
        EXPECT(create14(&v) == -1);
    }
    const snn_video_tensor_io good = io();
    for (int c : {0, 1, 2, 5}) EXPECT(create14(&good, 16, 12, c) == -1); // in_c outside {3, 4}
    for (const std::pair<int, int>& s : {std::pair<int, int>{63, 48}, {64, 47}, {0, 48}, {64, 0}, {-64, 48}, {64, -2}, {1, 1}}) // odd or non-positive src_w / src_h
        for (int f : {int(SNN_IO_NV12), int(SNN_IO_I420_16)}) {
            const snn_video_tensor_io v = io(f, SNN_IO_FLOAT, s.first, s.second, (f & 0x100) ? 1023 : 255);
            EXPECT(create14(&v) == -1);
        }
    EXPECT(create14(&good, 0, 12) == -1);
    EXPECT(create14(&good, 16, 0) == -1);
    EXPECT(create14(&good, -1, 12) == -1);
    EXPECT(create14(&good, 16, 12, 3, 0) == -1);
    EXPECT(create14(&good, 16, 12, 3, -1) == -1);
    for (const snn_video_tensor_io& v :
         {io(SNN_IO_NV12, 0, 64, 48, 255, 0, 1, 0, 0.299f, 0.114f, 2), io(SNN_IO_NV12, 0, 64, 48, 255, 0, 1, 0, 0.299f, 0.114f, -1), // an unknown filter
          io(SNN_IO_NV12, 0, 64, 48, 255, 0, 2), io(SNN_IO_NV12, 0, 64, 48, 255, 0, -1), io(SNN_IO_NV12, 0, 64, 48, 255, 0, 1, 2), io(SNN_IO_NV12, 0, 64, 48, 255, 0, 1, -1),
          io(SNN_IO_NV12, 0, 64, 48, 256), io(SNN_IO_NV12, 0, 64, 48, 127), io(SNN_IO_NV12, 0, 64, 48, 1023), io(SNN_IO_NV12, 0, 64, 48, 255, 1),
          io(SNN_IO_NV12_16, 0, 64, 48, 65535), io(SNN_IO_NV12_16, 0, 64, 48, 1023, 7), io(SNN_IO_I420_16, 0, 64, 48, 1000), io(SNN_IO_I420_16, 0, 64, 48, 8191),
          io(SNN_IO_I420, 0, 64, 48, 255, -1), io(SNN_IO_NV12, 0, 64, 48, 255, 0, 1, 0, 0.0f), io(SNN_IO_I420, 0, 64, 48, 255, 0, 1, 0, 0.299f, -0.1f),
          io(SNN_IO_NV12, 0, 64, 48, 255, 0, 1, 0, 0.7f, 0.3f)})
        EXPECT(create14(&v) == -1);

    // ---- the resolved line: the model is snn_model_create4's (snn_model_create5 with a null struct), or snn_model_create5's with the 8-bit output frame
    for (int c : {3, 4})
        for (int f : {int(SNN_IO_NV12), int(SNN_IO_NV12_16), int(SNN_IO_I420), int(SNN_IO_I420_16)}) {
            const snn_video_tensor_io v = io(f, SNN_IO_FLOAT, 1920, 1080, (f & 0x100) ? 1023 : 255, f == SNN_IO_NV12_16 ? 6 : 0);
            std::string rest;
            EXPECT(modelPart(14, &v, c, &rest) == modelPart(5, nullptr, c));
            EXPECT(rest.find("source=yuv420_tensor sink=model") != std::string::npos && rest.find("entry=snn_model_create14 | src=1920x1080 filter=1") != std::string::npos);
            EXPECT(rest.find((f == SNN_IO_I420 || f == SNN_IO_I420_16) ? "planar=1" : "planar=0") != std::string::npos);
        }
    {
        const snn_video_tensor_io v = io(SNN_IO_NV12, SNN_IO_RGB8);
        const snn_frame_io f{SNN_IO_FLOAT, SNN_IO_RGB8, {0, 0, 0, 0}, {1, 1, 1, 1}, {255, 255, 255, 255}, {0, 0, 0, 0}};
        EXPECT(modelPart(14, &v, 3) == modelPart(5, &f, 3));
    }

    if (failures) {
        fprintf(stderr, "yuv_tensor_host_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("yuv_tensor_host_check OK\n");
    return 0;
}
