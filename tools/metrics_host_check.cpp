// metrics_host_check.cpp -- the host paths of the frame-metrics feature that need no device, as a stand-alone program for a sanitizer build
// (DESIGN.md section 4.22): the null-argument refusals of the three model functions, the null-argument refusals of the C-ABI entry points, and
// snnhip_frame_metrics_psnr over its whole argument range (sse 0, 1, 2^64 - 1; pixels 0 .. 2^40; every depth).  Built against
// lib/libsnn_core_asan.so (python -c "import __graft_entry__ as g; g.build_host(sanitize='address,undefined')"):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Iinclude tools/metrics_host_check.cpp -o build/metrics_host_check \
//       -Lshadernn_amd/lib -lsnn_core_asan -lsnnhip -Wl,-rpath,$PWD/shadernn_amd/lib -Wl,-rpath,/opt/rocm/lib
// (tools/sanitize.sh checks builds and runs it with its siblings).  Exit status 0 and "metrics_host_check OK" when every expectation holds and the
// sanitizers stay silent.
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

int main() {
    unsigned char frame[64] = {0};
    const void* planes[3] = {frame, frame, frame};
    const int pitch[3] = {8, 4, 4};
    snn_frame_metrics rows[4];
    EXPECT(snn_model_reference_frame(nullptr, frame) == -1);
    EXPECT(snn_model_reference_frame(nullptr, nullptr) == -1);
    EXPECT(snn_model_reference_frame_planes(nullptr, planes, pitch, 3) == -1);
    EXPECT(snn_model_reference_frame_planes(nullptr, nullptr, nullptr, 0) == -1);
    EXPECT(snn_model_frame_metrics(nullptr, rows, 4) == -1);
    EXPECT(snn_model_frame_metrics(nullptr, nullptr, 0) == -1);
    EXPECT(sizeof(snn_frame_metrics) == 48 && sizeof(snnhip_frame_metrics_row) == 32 && sizeof(snnhip_frame_metrics_desc) == 28);

    snnhip_plan* plan = nullptr;
    snnhip_frame_metrics_desc desc{1, 16, 16, 1, SNNHIP_U8, 255, 0};
    snnhip_frame_metrics_row row;
    EXPECT(snnhip_frame_metrics_plan_create(nullptr, &desc, &plan) == SNNHIP_E_INVALID && plan == nullptr);
    EXPECT(snnhip_frame_metrics_read(nullptr, &row, 1) == SNNHIP_E_INVALID);

    EXPECT(std::isinf(snnhip_frame_metrics_psnr(0ull, 1920ull * 1080ull, 255)) && snnhip_frame_metrics_psnr(0ull, 1ull, 255) > 0);
    EXPECT(std::isinf(snnhip_frame_metrics_psnr(0ull, 0ull, 0)));
    EXPECT(std::fabs(snnhip_frame_metrics_psnr(100ull, 100ull, 255) - 20.0 * std::log10(255.0)) < 1e-12);
    const unsigned long long huge = ~0ull;
    for (int maxval : {1, 255, 1023, 4095, 65535})
        for (unsigned long long pixels : {1ull, 64ull, 3840ull * 2160ull, 1ull << 40}) {
            const double m = maxval, want = 10.0 * std::log10(m * m * static_cast<double>(pixels) / static_cast<double>(huge));
            const double got = snnhip_frame_metrics_psnr(huge, pixels, maxval);
            EXPECT(std::isfinite(got) && std::fabs(got - want) <= 1e-12 * std::fabs(want));
            // the largest squared error `pixels` samples of this depth can have: exactly 0 dB
            if (pixels <= (1ull << 32)) EXPECT(std::fabs(snnhip_frame_metrics_psnr(pixels * static_cast<unsigned long long>(maxval) * maxval, pixels, maxval)) < 1e-12);
        }
    EXPECT(snnhip_frame_metrics_psnr(1ull, 0ull, 255) < 0 && std::isinf(snnhip_frame_metrics_psnr(1ull, 0ull, 255))); // no pixels: log10(0), not a trap
    if (failures) {
        fprintf(stderr, "metrics_host_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("metrics_host_check OK\n");
    return 0;
}
