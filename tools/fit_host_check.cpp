// fit_host_check.cpp -- the host paths of the plane-fit feature that need no device, as a stand-alone program for a sanitizer build (DESIGN.md
// section 4.18): the tap table of one axis with its refusals, and every refusal of snn_model_create11 that returns before a model file is opened
// (what depends on the model's r -- a target above r * in or below r * in / 2 -- needs a device context and is
// tests/test_frame_fit_host_gpu.py's).  Built against lib/libsnn_core_asan.so (python -c "import __graft_entry__ as g;
// g.build_host(sanitize='address,undefined')"):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Iinclude tools/fit_host_check.cpp -o build/fit_host_check \
//       -Lshadernn_amd/lib -lsnn_core_asan -lsnnhip -Wl,-rpath,$PWD/shadernn_amd/lib -Wl,-rpath,/opt/rocm/lib
// Exit status 0 and "fit_host_check OK" when every expectation holds and the sanitizers stay silent.
#include <cmath>
#include <cstdio>
#include <initializer_list>
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

static snn_fit_io fit(int out_w, int out_h, int format = SNN_IO_NV12, int maxval = 255, int shift = 0, int siting = SNN_SITING_LEFT) {
    snn_fit_io io{};
    io.video.format = format;
    io.video.maxval = maxval;
    io.video.shift = shift;
    io.video.siting = siting;
    io.video.in_mean = 127.5f;
    io.video.in_norm = 1.0f / 127.5f;
    io.video.out_scale = 127.5f;
    io.video.out_offset = 127.5f;
    io.out_w = out_w;
    io.out_h = out_h;
    return io;
}

static int create11(const snn_fit_io* io, int w = 32, int h = 24, int in_c = 1, int batch = 1) {
    snn_model* m = nullptr;
    const int rc = snn_model_create11("no/such/model.json", 0, w, h, in_c, 0, 1, 0, 0, 0, batch, io, &m);
    EXPECT(m == nullptr);
    return rc;
}

int main() {
    // the table of one axis: [out][8] weights and [out] bases, written into buffers of exactly that size
    for (int siting : {SNNHIP_SITING_CENTRE, SNNHIP_SITING_LEFT})
        for (const std::pair<int, int>& io : {std::pair<int, int>{1, 1}, {3, 2}, {7, 5}, {4, 3}, {2562, 1920}, {100, 50}, {5, 20}, {9, 27}, {17, 17}, {2, 1}, {1, 4}}) {
            const int I = io.first, O = io.second;
            float* w = new float[8 * O];
            int* base = new int[O];
            EXPECT(snnhip_fit_taps(I, O, siting, w, base, 8 * O) == SNNHIP_OK);
            const long long a = siting == SNNHIP_SITING_LEFT ? 1 : 2;
            for (int X = 0; X < O; ++X) {
                const long long Nn = (4ll * X + a) * I - a * O, D = 4ll * O;
                EXPECT(base[X] == static_cast<int>(std::floor(static_cast<double>(Nn) / static_cast<double>(D))));
                EXPECT(X == 0 || (base[X] >= base[X - 1] && base[X] <= base[X - 1] + 2));
                double sum = 0.0;
                for (int k = 0; k < 8; ++k) sum += w[8 * X + k];
                EXPECT(std::fabs(sum - 1.0) <= 1e-6);
                if (O >= I) EXPECT(w[8 * X] == 0.0f && w[8 * X + 1] == 0.0f && w[8 * X + 6] == 0.0f && w[8 * X + 7] == 0.0f); // enlarging: the plain four-tap cubic
                if (O == I) EXPECT(base[X] == X && w[8 * X + 3] == 1.0f && w[8 * X + 2] == 0.0f && w[8 * X + 4] == 0.0f && w[8 * X + 5] == 0.0f); // a copy
            }
            EXPECT(snnhip_fit_taps(I, O, siting, w, base, 8 * O - 1) == SNNHIP_E_INVALID); // the capacity refusal: nothing is written past it
            delete[] w;
            delete[] base;
        }
    {
        float w[64];
        int base[8];
        EXPECT(snnhip_fit_taps(5, 2, 0, w, base, 64) == SNNHIP_E_INVALID); // below 1/2
        EXPECT(snnhip_fit_taps(2, 9, 0, w, base, 64) == SNNHIP_E_INVALID); // above 4 (the table would not fit either)
        EXPECT(snnhip_fit_taps(1, 5, 0, w, base, 64) == SNNHIP_E_INVALID);
        EXPECT(snnhip_fit_taps(0, 1, 0, w, base, 64) == SNNHIP_E_INVALID);
        EXPECT(snnhip_fit_taps(1, 0, 0, w, base, 64) == SNNHIP_E_INVALID);
        EXPECT(snnhip_fit_taps(-4, -4, 0, w, base, 64) == SNNHIP_E_INVALID);
        EXPECT(snnhip_fit_taps(4, 6, 2, w, base, 64) == SNNHIP_E_INVALID);
        EXPECT(snnhip_fit_taps(4, 6, -1, w, base, 64) == SNNHIP_E_INVALID);
        EXPECT(snnhip_fit_taps(4, 6, 1, nullptr, base, 64) == SNNHIP_E_INVALID);
        EXPECT(snnhip_fit_taps(4, 6, 1, w, nullptr, 64) == SNNHIP_E_INVALID);
        EXPECT(snnhip_fit_taps(4, 6, 1, w, base, 47) == SNNHIP_E_INVALID);
        EXPECT(snnhip_fit_taps(4, 6, 1, w, base, -1) == SNNHIP_E_INVALID);
        EXPECT(snnhip_fit_taps(4, 8, 1, w, base, 64) == SNNHIP_OK);
        EXPECT(snnhip_fit_taps(2, 1, 0, w, base, 8) == SNNHIP_OK); // exactly 1/2: all eight taps live, symmetric
        EXPECT(base[0] == 0 && w[0] != 0.0f && w[7] != 0.0f && w[0] == w[7] && w[3] == w[4]);
    }

    // snn_model_create11: everything it refuses before the model file is opened
    EXPECT(create11(nullptr) == -1);
    for (const std::pair<int, int>& o : {std::pair<int, int>{47, 36}, {48, 35}, {0, 36}, {48, 0}, {1, 1}, {-2, 36}, {48, -2}}) { // odd or below 2
        const snn_fit_io io = fit(o.first, o.second);
        EXPECT(create11(&io) == -1);
    }
    for (const std::pair<int, int>& o : {std::pair<int, int>{14, 36}, {130, 36}, {48, 10}, {48, 98}}) { // out / in outside [1/2, 4]
        const snn_fit_io io = fit(o.first, o.second);
        EXPECT(create11(&io) == -1);
    }
    const snn_fit_io good = fit(48, 36);
    EXPECT(create11(&good, 31, 24) == -1 && create11(&good, 32, 23) == -1 && create11(&good, 0, 24) == -1); // what snn_model_create8 refuses: the input extent ...
    EXPECT(create11(&good, 32, 24, 3) == -1 && create11(&good, 32, 24, 1, 0) == -1 && create11(&good, 32, 24, 1, -1) == -1); // ... channels and batch ...
    for (const snn_fit_io& io : {fit(48, 36, 0), fit(48, 36, SNN_IO_R8), fit(48, 36, SNN_IO_R16), fit(48, 36, SNN_IO_RGB8), fit(48, 36, SNN_IO_NV12, 256), fit(48, 36, SNN_IO_NV12, 0),
                                 fit(48, 36, SNN_IO_NV12, 255, 1), fit(48, 36, SNN_IO_NV12_16, 65535), fit(48, 36, SNN_IO_NV12_16, 1023, 7), fit(48, 36, SNN_IO_NV12_16, 1023, 16),
                                 fit(48, 36, SNN_IO_NV12, 255, 0, 2), fit(48, 36, SNN_IO_NV12, 255, 0, -1)}) // ... formats, depths and sitings
        EXPECT(create11(&io) == -1);
    if (failures) {
        fprintf(stderr, "fit_host_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("fit_host_check OK\n");
    return 0;
}
