// rgb_fit_host_check.cpp -- the host paths of the fitted-RGB feature that need no device, as a stand-alone program for a sanitizer build (DESIGN.md
// section 4.24): the four-tap table of one enlarging axis with its refusals, every refusal of snn_model_create13 that returns before a model file
// is opened, and the resolved lines against snn_model_create9's / snn_model_create7's (what depends on the model's r is
// tests/test_frame_rgb_fit_host_gpu.py's).  Built against lib/libsnn_core_asan.so by tools/sanitize.sh checks, as its siblings are.
// Exit status 0 and "rgb_fit_host_check OK" when every expectation holds and the sanitizers stay silent.
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

static snn_rgb_fit_io fit(int out_w, int out_h, int in_format = SNN_IO_NV12, int out_format = SNN_IO_RGB8, int maxval = 255, int shift = 0, int siting = SNN_SITING_LEFT,
                          int range = SNN_RANGE_LIMITED, float kr = 0.299f, float kb = 0.114f) {
    return snn_rgb_fit_io{in_format, out_format, maxval, shift, siting, range, kr, kb, out_w, out_h};
}

static int create13(const snn_rgb_fit_io* io, int w = 32, int h = 24, int in_c = 1, int batch = 1) {
    snn_model* m = nullptr;
    const int rc = snn_model_create13("no/such/model.json", 0, w, h, in_c, 0, 1, 0, 0, 0, batch, io, &m);
    EXPECT(m == nullptr);
    char line[1024];
    EXPECT(snn_frames_resolve(13, io, w, h, in_c, batch, line, sizeof(line)) == -1); // the resolver and the entry point refuse the same requests
    return rc;
}

// the part of a resolved line in front of the first " | ": the model
static std::string modelPart(int entry, const void* io, std::string* rest = nullptr) {
    char line[1024] = "";
    EXPECT(snn_frames_resolve(entry, io, 32, 24, 1, 1, line, sizeof(line)) == 0);
    const std::string s(line);
    const size_t bar = s.find(" | ");
    EXPECT(bar != std::string::npos);
    if (rest) *rest = bar == std::string::npos ? std::string() : s.substr(bar);
    return s.substr(0, bar);
}

int main() {
    // the table of one axis: [out][4] weights and [out] bases, written into buffers of exactly that size
    for (int siting : {SNNHIP_SITING_CENTRE, SNNHIP_SITING_LEFT})
        for (const std::pair<int, int>& io : {std::pair<int, int>{1, 1}, {1, 8}, {2, 4}, {3, 5}, {5, 13}, {7, 19}, {35, 100}, {360, 1080}, {640, 1920}, {17, 17}, {70, 141}}) {
            const int I = io.first, O = io.second;
            float* w = new float[4 * O];
            int* base = new int[O];
            EXPECT(snnhip_rgb_fit_taps(I, O, siting, w, base, 4 * O) == SNNHIP_OK);
            const long long a = siting == SNNHIP_SITING_LEFT ? 1 : 2;
            for (int X = 0; X < O; ++X) {
                const long long Nn = (4ll * X + 2) * I - a * O, D = 4ll * O;
                EXPECT(base[X] == static_cast<int>(std::floor(static_cast<double>(Nn) / static_cast<double>(D))));
                EXPECT(X == 0 || (base[X] >= base[X - 1] && base[X] <= base[X - 1] + 1));
                EXPECT(base[X] >= -1 && base[X] <= I - 1);
                double sum = 0.0;
                for (int k = 0; k < 4; ++k) sum += w[4 * X + k];
                EXPECT(std::fabs(sum - 1.0) <= 1e-6);
                if (O == I && siting == SNNHIP_SITING_CENTRE) EXPECT(base[X] == X && w[4 * X + 1] == 1.0f && w[4 * X] == 0.0f && w[4 * X + 2] == 0.0f && w[4 * X + 3] == 0.0f);
            }
            EXPECT(snnhip_rgb_fit_taps(I, O, siting, w, base, 4 * O - 1) == SNNHIP_E_INVALID); // the capacity refusal: nothing is written past it
            delete[] w;
            delete[] base;
        }
    for (int r = 1; r <= 4; ++r) // an integer factor of a chroma plane: the bases of the fixed-phase table of yuv_rgb
        for (int siting : {SNNHIP_SITING_CENTRE, SNNHIP_SITING_LEFT}) {
            float w[8 * 4 * 3], w420[32];
            int base[8 * 3], base420[8];
            EXPECT(snnhip_rgb_fit_taps(3, 2 * r * 3, siting, w, base, 8 * 4 * 3) == SNNHIP_OK);
            EXPECT(snnhip_bicubic_taps_420(r, siting, w420, base420, 32) == SNNHIP_OK);
            for (int X = 0; X < 2 * r * 3; ++X) {
                EXPECT(base[X] == X / (2 * r) + base420[X % (2 * r)]);
                for (int k = 0; k < 4; ++k) EXPECT(std::fabs(w[4 * X + k] - w420[4 * (X % (2 * r)) + k]) <= 1.2e-7f);
            }
        }
    {
        float w[64];
        int base[16];
        EXPECT(snnhip_rgb_fit_taps(5, 4, 0, w, base, 64) == SNNHIP_E_INVALID); // below 1
        EXPECT(snnhip_rgb_fit_taps(1, 9, 0, w, base, 64) == SNNHIP_E_INVALID); // above 8
        EXPECT(snnhip_rgb_fit_taps(0, 1, 0, w, base, 64) == SNNHIP_E_INVALID);
        EXPECT(snnhip_rgb_fit_taps(1, 0, 0, w, base, 64) == SNNHIP_E_INVALID);
        EXPECT(snnhip_rgb_fit_taps(-4, -4, 0, w, base, 64) == SNNHIP_E_INVALID);
        EXPECT(snnhip_rgb_fit_taps(4, 6, 2, w, base, 64) == SNNHIP_E_INVALID);
        EXPECT(snnhip_rgb_fit_taps(4, 6, -1, w, base, 64) == SNNHIP_E_INVALID);
        EXPECT(snnhip_rgb_fit_taps(4, 6, 1, nullptr, base, 64) == SNNHIP_E_INVALID);
        EXPECT(snnhip_rgb_fit_taps(4, 6, 1, w, nullptr, 64) == SNNHIP_E_INVALID);
        EXPECT(snnhip_rgb_fit_taps(4, 6, 1, w, base, 23) == SNNHIP_E_INVALID);
        EXPECT(snnhip_rgb_fit_taps(4, 6, 1, w, base, -1) == SNNHIP_E_INVALID);
        EXPECT(snnhip_rgb_fit_taps(2, 16, 1, w, base, 64) == SNNHIP_OK); // exactly 8
        EXPECT(snnhip_rgb_fit_taps(16, 16, 0, w, base, 64) == SNNHIP_OK); // exactly 1
    }

    // snn_model_create13: everything it refuses before the model file is opened
    EXPECT(create13(nullptr) == -1);
    for (const std::pair<int, int>& f : {std::pair<int, int>{SNN_IO_NV12, SNN_IO_RGB16}, {SNN_IO_NV12, SNN_IO_NV12}, {SNN_IO_NV12, SNN_IO_R8}, {SNN_IO_NV12, 0}, {SNN_IO_NV12_16, SNN_IO_RGB8},
                                         {SNN_IO_I420, SNN_IO_RGBA16}, {SNN_IO_I420, SNN_IO_I420}, {SNN_IO_I420_16, SNN_IO_RGBA8}, {SNN_IO_RGB8, SNN_IO_RGBA8}, {SNN_IO_RGBA8, SNN_IO_RGB8},
                                         {SNN_IO_RGB8, SNN_IO_NV12}, {SNN_IO_RGB16, SNN_IO_RGB16}, {SNN_IO_R8, SNN_IO_R8}, {0, SNN_IO_RGB8}}) { // formats that do not pair up
        const snn_rgb_fit_io io = fit(48, 36, f.first, f.second, (f.first & 0x100) ? 1023 : 255);
        EXPECT(create13(&io) == -1);
    }
    for (const std::pair<int, int>& o : {std::pair<int, int>{0, 36}, {48, 0}, {-2, 36}, {48, -1}, {15, 36}, {129, 36}, {48, 11}, {48, 97}}) { // below 1; video: outside [1/2, 4]
        const snn_rgb_fit_io io = fit(o.first, o.second);
        EXPECT(create13(&io) == -1);
    }
    for (const std::pair<int, int>& o : {std::pair<int, int>{0, 36}, {31, 36}, {129, 36}, {48, 23}, {48, 97}, {16, 12}}) { // a colour frame: outside [1, 4]
        const snn_rgb_fit_io io = fit(o.first, o.second, SNN_IO_RGBA8, SNN_IO_RGBA8);
        EXPECT(create13(&io) == -1);
    }
    const snn_rgb_fit_io good = fit(47, 35);
    EXPECT(create13(&good, 31, 24) == -1 && create13(&good, 32, 23) == -1 && create13(&good, 0, 24) == -1); // what snn_model_create9 refuses: the input extent ...
    EXPECT(create13(&good, 32, 24, 3) == -1 && create13(&good, 32, 24, 1, 0) == -1 && create13(&good, 32, 24, 1, -1) == -1); // ... channels and batch ...
    for (const snn_rgb_fit_io& io : {fit(48, 36, SNN_IO_NV12, SNN_IO_RGB8, 256), fit(48, 36, SNN_IO_NV12, SNN_IO_RGB8, 127), fit(48, 36, SNN_IO_NV12, SNN_IO_RGB8, 255, 1),
                                     fit(48, 36, SNN_IO_NV12_16, SNN_IO_RGB16, 65535), fit(48, 36, SNN_IO_NV12_16, SNN_IO_RGB16, 1023, 7), fit(48, 36, SNN_IO_I420_16, SNN_IO_RGB16, 1000),
                                     fit(48, 36, SNN_IO_NV12, SNN_IO_RGB8, 255, 0, 2), fit(48, 36, SNN_IO_I420, SNN_IO_RGB8, 255, 0, -1), fit(48, 36, SNN_IO_NV12, SNN_IO_RGB8, 255, 0, 1, 2),
                                     fit(48, 36, SNN_IO_NV12, SNN_IO_RGB8, 255, 0, 1, 0, 0.0f), fit(48, 36, SNN_IO_I420, SNN_IO_RGB8, 255, 0, 1, 0, 0.299f, -0.1f),
                                     fit(48, 36, SNN_IO_RGB8, SNN_IO_RGB8, 255, 0, 1, 0, 0.7f, 0.3f)}) // ... depths, sitings, ranges and matrices
        EXPECT(create13(&io) == -1);
    const snn_rgb_fit_io colour = fit(48, 36, SNN_IO_RGB8, SNN_IO_RGB8);
    EXPECT(create13(&colour, 32, 24, 3) == -1 && create13(&colour, 32, 24, 1, 0) == -1); // what snn_model_create7 refuses

    // the model of a resolved request is snn_model_create9's (video in) or snn_model_create7's with the full-range luma maps (a colour frame in)
    for (const std::pair<int, int>& f : {std::pair<int, int>{SNN_IO_NV12, SNN_IO_RGB8}, {SNN_IO_NV12, SNN_IO_RGBA8}, {SNN_IO_NV12_16, SNN_IO_RGB16}, {SNN_IO_I420, SNN_IO_RGBA8},
                                         {SNN_IO_I420_16, SNN_IO_RGB16}})
        for (int range : {SNN_RANGE_LIMITED, SNN_RANGE_FULL}) {
            const bool wide = (f.first & 0x100) != 0, planar = f.first == SNN_IO_I420 || f.first == SNN_IO_I420_16;
            const snn_rgb_fit_io io = fit(47, 35, f.first, f.second, wide ? 1023 : 255, 0, SNN_SITING_LEFT, range);
            const snn_video_rgb_io v{wide ? int(SNN_IO_NV12_16) : int(SNN_IO_NV12), f.second, io.maxval, 0, SNN_SITING_LEFT, range, io.kr, io.kb};
            std::string rest;
            EXPECT(modelPart(13, &io, &rest) == modelPart(9, &v));
            EXPECT(rest.find("sink=rgb_from_yuv_fitted") != std::string::npos && rest.find("fit=47x35") != std::string::npos);
            EXPECT(rest.find(planar ? "planar=1" : "planar=0") != std::string::npos && rest.find("entry=snn_model_create13") != std::string::npos);
        }
    for (int format : {int(SNN_IO_RGB8), int(SNN_IO_RGBA8)}) {
        const snn_rgb_fit_io io = fit(47, 35, format, format);
        const snn_colour_io c{format, io.kr, io.kb, 0.0f, 1.0f / 255.0f, 255.0f, 0.0f};
        std::string rest;
        EXPECT(modelPart(13, &io, &rest) == modelPart(7, &c));
        EXPECT(rest.find("sink=rgb_merged_fitted") != std::string::npos && rest.find("fit=47x35") != std::string::npos && rest.find("entry=snn_model_create13") != std::string::npos);
    }
    if (failures) {
        fprintf(stderr, "rgb_fit_host_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("rgb_fit_host_check OK\n");
    return 0;
}
