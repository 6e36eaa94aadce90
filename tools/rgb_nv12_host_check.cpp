// rgb_nv12_host_check.cpp -- the host paths of the RGB -> NV12 feature that need no device, as a stand-alone program for a sanitizer build (DESIGN.md
// section 4.17): the tap table of the upscaled frame's chroma grid and the chroma scale table with their refusals, and every refusal of
// snn_model_create10 that returns before a model file is opened (what depends on the model's r -- r outside 2..4, an odd r * in_w -- needs a device
// context and is tests/test_frame_rgb_cbcr_host_gpu.py's).  Built against lib/libsnn_core_asan.so (python -c "import __graft_entry__ as g;
// g.build_host(sanitize='address,undefined')"):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Iinclude tools/rgb_nv12_host_check.cpp -o build/rgb_nv12_host_check \
//       -Lshadernn_amd/lib -lsnn_core_asan -lsnnhip -Wl,-rpath,$PWD/shadernn_amd/lib -Wl,-rpath,/opt/rocm/lib
// Exit status 0 and "rgb_nv12_host_check OK" when every expectation holds and the sanitizers stay silent.
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

static int create10(const snn_encode_io* io, int w = 32, int h = 24, int in_c = 1, int batch = 1) {
    snn_model* m = nullptr;
    const int rc = snn_model_create10("no/such/model.json", 0, w, h, in_c, 0, 1, 0, 0, 0, batch, io, &m);
    EXPECT(m == nullptr);
    return rc;
}

static snn_encode_io encode(int in_format = SNN_IO_RGB8, int out_format = SNN_IO_NV12, int siting = SNN_SITING_LEFT, int range = SNN_RANGE_LIMITED, float kr = 0.299f,
                            float kb = 0.114f) {
    snn_encode_io io{};
    io.in_format = in_format;
    io.out_format = out_format;
    io.siting = siting;
    io.range = range;
    io.kr = kr;
    io.kb = kb;
    return io;
}

static bool close_to(double got, double want, double rel = 1e-6) { return std::fabs(got - want) <= rel * std::fabs(want) + 1e-12; }

int main() {
    // the tap table: [P][4] weights and [P] bases, P = 1, 3, 2 for r = 2, 3, 4, written into buffers of exactly that size
    for (int siting : {SNNHIP_SITING_CENTRE, SNNHIP_SITING_LEFT})
        for (int r = 2; r <= 4; ++r) {
            const int P = r % 2 ? r : r / 2;
            float* w = new float[4 * P];
            int* base = new int[P];
            EXPECT(snnhip_bicubic_taps_rgb420(r, siting, w, base, 4 * P) == SNNHIP_OK);
            for (int p = 0; p < P; ++p) {
                const double lead = siting == SNNHIP_SITING_LEFT ? 0.5 : 1.0;
                EXPECT(base[p] == static_cast<int>(std::floor((2 * p + lead) / r - 0.5)));
                EXPECT(base[p] >= -1 && base[p] <= 1);
                double sum = 0.0;
                for (int k = 0; k < 4; ++k) sum += w[4 * p + k];
                EXPECT(std::fabs(sum - 1.0) <= 1.2e-7);
            }
            EXPECT(snnhip_bicubic_taps_rgb420(r, siting, w, base, 4 * P - 1) == SNNHIP_E_INVALID); // the capacity refusal: nothing is written past it
            delete[] w;
            delete[] base;
        }
    {
        float w[12];
        int base[3];
        EXPECT(snnhip_bicubic_taps_rgb420(2, SNNHIP_SITING_CENTRE, w, base, 4) == SNNHIP_OK); // the identity
        EXPECT(base[0] == 0 && w[0] == 0.0f && w[1] == 1.0f && w[2] == 0.0f && w[3] == 0.0f);
        EXPECT(snnhip_bicubic_taps_rgb420(2, SNNHIP_SITING_LEFT, w, base, 4) == SNNHIP_OK); // a quarter-pixel shift
        EXPECT(base[0] == -1 && close_to(w[0], -0.0234375) && close_to(w[1], 0.2265625) && close_to(w[2], 0.8671875) && close_to(w[3], -0.0703125));
        EXPECT(snnhip_bicubic_taps_rgb420(3, SNNHIP_SITING_LEFT, w, base, 12) == SNNHIP_OK); // phase 2: the identity on input 2x' + 1
        EXPECT(base[2] == 1 && w[8] == 0.0f && w[9] == 1.0f && w[10] == 0.0f && w[11] == 0.0f);
        EXPECT(snnhip_bicubic_taps_rgb420(0, 1, w, base, 12) == SNNHIP_E_INVALID);
        EXPECT(snnhip_bicubic_taps_rgb420(1, 1, w, base, 12) == SNNHIP_E_INVALID); // r = 1 would decimate
        EXPECT(snnhip_bicubic_taps_rgb420(5, 1, w, base, 12) == SNNHIP_E_INVALID);
        EXPECT(snnhip_bicubic_taps_rgb420(2, 2, w, base, 12) == SNNHIP_E_INVALID);
        EXPECT(snnhip_bicubic_taps_rgb420(2, -1, w, base, 12) == SNNHIP_E_INVALID);
        EXPECT(snnhip_bicubic_taps_rgb420(2, 1, nullptr, base, 12) == SNNHIP_E_INVALID);
        EXPECT(snnhip_bicubic_taps_rgb420(2, 1, w, nullptr, 12) == SNNHIP_E_INVALID);
    }

    // the coefficient table: Coff, cbs, crs; cbs and crs invert yuv_rgb's cbu and crv
    for (int range : {SNNHIP_RANGE_LIMITED, SNNHIP_RANGE_FULL}) {
        float c[3], back[7];
        const float kr = 0.2126f, kb = 0.0722f;
        EXPECT(snnhip_rgb_cbcr_coefficients(range, kr, kb, c, 3) == SNNHIP_OK);
        const double crange = range == SNNHIP_RANGE_LIMITED ? 224.0 : 255.0;
        EXPECT(c[0] == 128.0f);
        EXPECT(close_to(c[1], crange / (2.0 * (1.0 - kb) * 255.0)) && close_to(c[2], crange / (2.0 * (1.0 - kr) * 255.0)));
        EXPECT(snnhip_yuv_rgb_coefficients(255, range, kr, kb, back, 7) == SNNHIP_OK);
        EXPECT(close_to(static_cast<double>(c[1]) * back[4], 1.0, 3e-7) && close_to(static_cast<double>(c[2]) * back[3], 1.0, 3e-7));
    }
    {
        float c[3];
        EXPECT(snnhip_rgb_cbcr_coefficients(0, 0.299f, 0.114f, c, 2) == SNNHIP_E_INVALID);
        EXPECT(snnhip_rgb_cbcr_coefficients(0, 0.299f, 0.114f, nullptr, 3) == SNNHIP_E_INVALID);
        EXPECT(snnhip_rgb_cbcr_coefficients(2, 0.299f, 0.114f, c, 3) == SNNHIP_E_INVALID);
        EXPECT(snnhip_rgb_cbcr_coefficients(-1, 0.299f, 0.114f, c, 3) == SNNHIP_E_INVALID);
        EXPECT(snnhip_rgb_cbcr_coefficients(0, 0.0f, 0.114f, c, 3) == SNNHIP_E_INVALID);
        EXPECT(snnhip_rgb_cbcr_coefficients(0, 0.299f, 0.0f, c, 3) == SNNHIP_E_INVALID);
        EXPECT(snnhip_rgb_cbcr_coefficients(0, 0.7f, 0.3f, c, 3) == SNNHIP_E_INVALID);
        EXPECT(snnhip_rgb_cbcr_coefficients(0, 0.299f, 0.114f, c, 3) == SNNHIP_OK);
        EXPECT(close_to(c[1], 224.0 / 255.0 / 1.772) && close_to(c[2], 224.0 / 255.0 / 1.402));
    }

    // snn_model_create10: everything it refuses before the model file is opened
    EXPECT(create10(nullptr) == -1);
    for (int fmt : {0, 1, 5, 0x103, 0x104, 0x201, 0x301}) {
        const snn_encode_io io = encode(fmt);
        EXPECT(create10(&io) == -1);
    }
    for (int out : {0, 1, 3, 4, 0x103, 0x301}) { // NV12 only
        const snn_encode_io io = encode(SNN_IO_RGB8, out);
        EXPECT(create10(&io) == -1);
    }
    const snn_encode_io rgb = encode(), rgba = encode(SNN_IO_RGBA8);
    EXPECT(create10(&rgb, 32, 24, 3) == -1); // the model takes one channel whatever the frame has
    EXPECT(create10(&rgba, 32, 24, 4) == -1);
    EXPECT(create10(&rgb, 32, 24, 1, 0) == -1);
    EXPECT(create10(&rgb, 32, 24, 1, -1) == -1);
    for (const snn_encode_io& io : {encode(SNN_IO_RGB8, SNN_IO_NV12, 2), encode(SNN_IO_RGB8, SNN_IO_NV12, -1), encode(SNN_IO_RGB8, SNN_IO_NV12, 1, 2),
                                    encode(SNN_IO_RGB8, SNN_IO_NV12, 1, -1), encode(SNN_IO_RGB8, SNN_IO_NV12, 1, 0, 0.0f), encode(SNN_IO_RGB8, SNN_IO_NV12, 1, 0, 0.299f, 0.0f),
                                    encode(SNN_IO_RGB8, SNN_IO_NV12, 1, 0, 0.7f, 0.3f), encode(SNN_IO_RGBA8, SNN_IO_NV12, 0, 1, -0.1f, 0.114f)})
        EXPECT(create10(&io) == -1);
    if (failures) {
        fprintf(stderr, "rgb_nv12_host_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("rgb_nv12_host_check OK\n");
    return 0;
}
