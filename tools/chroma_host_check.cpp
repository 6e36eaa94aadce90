// chroma_host_check.cpp -- the host paths of the NV12 / P010 feature that need no device, as a stand-alone program for a sanitizer build
// (DESIGN.md section 4.14): every refusal of snn_model_create8 that returns before a model file is opened, the two frame calls on a null model,
// and the sited tap table with its refusals.  Built against lib/libsnn_core_asan.so (python -c "import __graft_entry__ as g;
// g.build_host(sanitize='address,undefined')"):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Iinclude tools/chroma_host_check.cpp -o build/chroma_host_check \
//       -Lshadernn_amd/lib -lsnn_core_asan -lsnnhip -Wl,-rpath,$PWD/shadernn_amd/lib -Wl,-rpath,/opt/rocm/lib
// Exit status 0 and "chroma_host_check OK" when every expectation holds and the sanitizers stay silent.
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

static int create8(const snn_video_io* io, int w = 32, int h = 24, int in_c = 1, int batch = 1) {
    snn_model* m = nullptr;
    const int rc = snn_model_create8("no/such/model.json", 0, w, h, in_c, 0, 1, 0, 0, 0, batch, io, &m);
    EXPECT(m == nullptr);
    return rc;
}

static snn_video_io video(int format, int maxval, int shift, int siting) {
    snn_video_io io{};
    io.format = format;
    io.maxval = maxval;
    io.shift = shift;
    io.siting = siting;
    io.in_norm = 1.0f / static_cast<float>(maxval);
    io.out_scale = static_cast<float>(maxval);
    return io;
}

int main() {
    EXPECT(create8(nullptr) == -1);
    for (int fmt : {0, 1, 3, 4, 0x101, 0x202}) {
        const snn_video_io io = video(fmt, 255, 0, SNN_SITING_LEFT);
        EXPECT(create8(&io) == -1);
    }
    const snn_video_io nv12 = video(SNN_IO_NV12, 255, 0, SNN_SITING_LEFT);
    EXPECT(create8(&nv12, 32, 24, 3) == -1);
    EXPECT(create8(&nv12, 31, 24) == -1);
    EXPECT(create8(&nv12, 32, 23) == -1);
    EXPECT(create8(&nv12, 32, 24, 1, 0) == -1);
    for (const snn_video_io& io : {video(SNN_IO_NV12_16, 65535, 0, 1), video(SNN_IO_NV12_16, 4096, 0, 1), video(SNN_IO_NV12_16, 1023, 7, 1), video(SNN_IO_NV12, 1023, 0, 1),
                                   video(SNN_IO_NV12, 127, 1, 1), video(SNN_IO_NV12, 255, 0, 2), video(SNN_IO_NV12, 0, 0, 1), video(SNN_IO_NV12_16, 1023, -1, 1)})
        EXPECT(create8(&io) == -1);
    EXPECT(snn_model_upload_frame_nv12(nullptr, nullptr) == -1);
    EXPECT(snn_model_download_frame_nv12(nullptr, nullptr) == -1);

    for (int siting : {SNNHIP_SITING_CENTRE, SNNHIP_SITING_LEFT})
        for (int r = 1; r <= 4; ++r) {
            float w[16];
            int base[4];
            EXPECT(snnhip_bicubic_taps_sited(r, siting, w, base, 4 * r) == SNNHIP_OK);
            for (int p = 0; p < r; ++p) {
                const double off = siting == SNNHIP_SITING_LEFT ? 0.25 : 0.5;
                EXPECT(base[p] == static_cast<int>(std::floor((p + off) / r - off)));
                double sum = 0.0;
                for (int k = 0; k < 4; ++k) sum += w[4 * p + k];
                EXPECT(std::fabs(sum - 1.0) <= 1.2e-7);
            }
            EXPECT(snnhip_bicubic_taps_sited(r, siting, w, base, 4 * r - 1) == SNNHIP_E_INVALID);
        }
    float w[16];
    int base[4];
    EXPECT(snnhip_bicubic_taps_sited(0, 1, w, base, 16) == SNNHIP_E_INVALID);
    EXPECT(snnhip_bicubic_taps_sited(5, 1, w, base, 16) == SNNHIP_E_INVALID);
    EXPECT(snnhip_bicubic_taps_sited(2, 2, w, base, 16) == SNNHIP_E_INVALID);
    EXPECT(snnhip_bicubic_taps_sited(2, 1, nullptr, base, 16) == SNNHIP_E_INVALID);
    EXPECT(snnhip_bicubic_taps_sited(2, 1, w, nullptr, 16) == SNNHIP_E_INVALID);
    if (failures) {
        fprintf(stderr, "chroma_host_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("chroma_host_check OK\n");
    return 0;
}
