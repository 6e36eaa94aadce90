// video_rgb_host_check.cpp -- the host paths of the NV12 / P010 -> RGB feature that need no device, as a stand-alone program for a sanitizer build
// (DESIGN.md section 4.15): the 4:2:0 tap table and the matrix coefficient table with their refusals, and every refusal of snn_model_create9 that
// returns before a model file is opened.  Built against lib/libsnn_core_asan.so (python -c "import __graft_entry__ as g;
// g.build_host(sanitize='address,undefined')"):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Iinclude tools/video_rgb_host_check.cpp -o build/video_rgb_host_check \
//       -Lshadernn_amd/lib -lsnn_core_asan -lsnnhip -Wl,-rpath,$PWD/shadernn_amd/lib -Wl,-rpath,/opt/rocm/lib
// Exit status 0 and "video_rgb_host_check OK" when every expectation holds and the sanitizers stay silent.
#include <cmath>
#include <cstdio>
#include <initializer_list>

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

static int create9(const snn_video_rgb_io* io, int w = 32, int h = 24, int in_c = 1, int batch = 1) {
    snn_model* m = nullptr;
    const int rc = snn_model_create9("no/such/model.json", 0, w, h, in_c, 0, 1, 0, 0, 0, batch, io, &m);
    EXPECT(m == nullptr);
    return rc;
}

static snn_video_rgb_io video(int in_format, int out_format, int maxval = 255, int shift = 0, int siting = SNN_SITING_LEFT, int range = SNN_RANGE_LIMITED, float kr = 0.299f,
                              float kb = 0.114f) {
    snn_video_rgb_io io{};
    io.in_format = in_format;
    io.out_format = out_format;
    io.maxval = maxval;
    io.shift = shift;
    io.siting = siting;
    io.range = range;
    io.kr = kr;
    io.kb = kb;
    return io;
}

static bool close_to(double got, double want, double rel = 1e-6) { return std::fabs(got - want) <= rel * std::fabs(want) + 1e-12; }

int main() {
    // the 4:2:0 tap table: [2r][4] weights and [2r] bases
    for (int siting : {SNNHIP_SITING_CENTRE, SNNHIP_SITING_LEFT})
        for (int r = 1; r <= 4; ++r) {
            float w[32];
            int base[8];
            EXPECT(snnhip_bicubic_taps_420(r, siting, w, base, 8 * r) == SNNHIP_OK);
            for (int p = 0; p < 2 * r; ++p) {
                const double off = siting == SNNHIP_SITING_LEFT ? 0.25 : 0.5;
                EXPECT(base[p] == static_cast<int>(std::floor((p + 0.5) / (2 * r) - off)));
                EXPECT(base[p] == -1 || base[p] == 0);
                double sum = 0.0;
                for (int k = 0; k < 4; ++k) sum += w[4 * p + k];
                EXPECT(std::fabs(sum - 1.0) <= 1.2e-7);
            }
            EXPECT(snnhip_bicubic_taps_420(r, siting, w, base, 8 * r - 1) == SNNHIP_E_INVALID); // the capacity refusal: nothing is written past it
        }
    {
        float w[32];
        int base[8];
        EXPECT(snnhip_bicubic_taps_420(0, 1, w, base, 32) == SNNHIP_E_INVALID);
        EXPECT(snnhip_bicubic_taps_420(5, 1, w, base, 32) == SNNHIP_E_INVALID);
        EXPECT(snnhip_bicubic_taps_420(2, 2, w, base, 32) == SNNHIP_E_INVALID);
        EXPECT(snnhip_bicubic_taps_420(2, 1, nullptr, base, 32) == SNNHIP_E_INVALID);
        EXPECT(snnhip_bicubic_taps_420(2, 1, w, nullptr, 32) == SNNHIP_E_INVALID);
    }

    // the coefficient table: Yoff, Coff, cy, crv, cbu, cgv, cgu
    for (int maxval : {255, 1023, 4095}) {
        const double k = (maxval + 1) / 256.0, m = maxval;
        for (int range : {SNNHIP_RANGE_LIMITED, SNNHIP_RANGE_FULL}) {
            float c[7];
            const float kr = 0.2126f, kb = 0.0722f;
            EXPECT(snnhip_yuv_rgb_coefficients(maxval, range, kr, kb, c, 7) == SNNHIP_OK);
            const double yrange = range == SNNHIP_RANGE_LIMITED ? 219.0 * k : m, crange = range == SNNHIP_RANGE_LIMITED ? 224.0 * k : m;
            const double kg = 1.0 - kr - kb, crv = 2.0 * (1.0 - kr) * m / crange, cbu = 2.0 * (1.0 - kb) * m / crange;
            EXPECT(c[0] == static_cast<float>(range == SNNHIP_RANGE_LIMITED ? 16.0 * k : 0.0));
            EXPECT(c[1] == static_cast<float>(128.0 * k));
            EXPECT(close_to(c[2], m / yrange) && close_to(c[3], crv) && close_to(c[4], cbu) && close_to(c[5], kr * crv / kg) && close_to(c[6], kb * cbu / kg));
        }
    }
    {
        float c[7];
        EXPECT(snnhip_yuv_rgb_coefficients(255, 0, 0.299f, 0.114f, c, 6) == SNNHIP_E_INVALID);
        EXPECT(snnhip_yuv_rgb_coefficients(255, 0, 0.299f, 0.114f, nullptr, 7) == SNNHIP_E_INVALID);
        EXPECT(snnhip_yuv_rgb_coefficients(256, 0, 0.299f, 0.114f, c, 7) == SNNHIP_E_INVALID);
        EXPECT(snnhip_yuv_rgb_coefficients(255, 2, 0.299f, 0.114f, c, 7) == SNNHIP_E_INVALID);
        EXPECT(snnhip_yuv_rgb_coefficients(255, 0, 0.0f, 0.114f, c, 7) == SNNHIP_E_INVALID);
        EXPECT(snnhip_yuv_rgb_coefficients(255, 0, 0.7f, 0.3f, c, 7) == SNNHIP_E_INVALID);
        EXPECT(snnhip_yuv_rgb_coefficients(255, 0, 0.299f, 0.114f, c, 7) == SNNHIP_OK);
        EXPECT(close_to(c[2], 255.0 / 219.0) && close_to(c[3], 1.596027) && close_to(c[4], 2.017232) && close_to(c[5], 0.812968) && close_to(c[6], 0.391762));
    }

    // snn_model_create9: everything it refuses before the model file is opened
    EXPECT(create9(nullptr) == -1);
    for (int fmt : {0, 1, 3, 4, 0x101, 0x202}) {
        const snn_video_rgb_io io = video(fmt, SNN_IO_RGB8);
        EXPECT(create9(&io) == -1);
    }
    for (int out : {0, 1, 0x103, 0x104, 0x201}) { // an 8-bit input pairs with RGB8 / RGBA8 only
        const snn_video_rgb_io io = video(SNN_IO_NV12, out);
        EXPECT(create9(&io) == -1);
    }
    for (int out : {3, 4, 0x101, 0x301}) { // ... a 16-bit one with RGB16 / RGBA16 only
        const snn_video_rgb_io io = video(SNN_IO_NV12_16, out, 1023, 6);
        EXPECT(create9(&io) == -1);
    }
    const snn_video_rgb_io nv12 = video(SNN_IO_NV12, SNN_IO_RGBA8);
    EXPECT(create9(&nv12, 32, 24, 3) == -1);
    EXPECT(create9(&nv12, 31, 24) == -1);
    EXPECT(create9(&nv12, 32, 23) == -1);
    EXPECT(create9(&nv12, 32, 24, 1, 0) == -1);
    for (const snn_video_rgb_io& io :
         {video(SNN_IO_NV12_16, SNN_IO_RGB16, 65535), video(SNN_IO_NV12_16, SNN_IO_RGB16, 8191), video(SNN_IO_NV12_16, SNN_IO_RGB16, 1023, 7), video(SNN_IO_NV12, SNN_IO_RGB8, 1023),
          video(SNN_IO_NV12, SNN_IO_RGB8, 127), video(SNN_IO_NV12_16, SNN_IO_RGB16, 1000), video(SNN_IO_NV12, SNN_IO_RGB8, 255, 1), video(SNN_IO_NV12_16, SNN_IO_RGB16, 1023, -1),
          video(SNN_IO_NV12, SNN_IO_RGB8, 255, 0, 2), video(SNN_IO_NV12, SNN_IO_RGB8, 255, 0, 1, 2), video(SNN_IO_NV12, SNN_IO_RGB8, 255, 0, 1, -1),
          video(SNN_IO_NV12, SNN_IO_RGB8, 255, 0, 1, 0, 0.0f), video(SNN_IO_NV12, SNN_IO_RGB8, 255, 0, 1, 0, 0.299f, 0.0f), video(SNN_IO_NV12, SNN_IO_RGB8, 255, 0, 1, 0, 0.7f, 0.3f)})
        EXPECT(create9(&io) == -1);
    if (failures) {
        fprintf(stderr, "video_rgb_host_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("video_rgb_host_check OK\n");
    return 0;
}
