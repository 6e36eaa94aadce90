// frames_host_check.cpp -- the frame description behind snn_model_create5 .. 12 (shadernn_amd/host/snn/frames.h) as a
// stand-alone program for a sanitizer build: through snn_frames_resolve, every "built exactly as" statement of include/snn_c.h (the resolved model
// lines are equal), every snn_model_create12 path against its NV12 counterpart (equal but for the planar flag and the entry name), and the refusals
// of every entry point's own rules -- what tests/test_frame_paths.py expects, here on stack and heap structs of exactly their size, so that a
// resolver reading past its struct (a snn_frame_io taken for a snn_frame_io2, say) is an error the sanitizer reports.  Built against
// lib/libsnn_core_asan.so (python -c "import __graft_entry__ as g; g.build_host(sanitize='address,undefined')"):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Iinclude tools/frames_host_check.cpp -o build/frames_host_check \
//       -Lshadernn_amd/lib -lsnn_core_asan -lsnnhip -Wl,-rpath,$PWD/shadernn_amd/lib -Wl,-rpath,/opt/rocm/lib
// Exit status 0 and "frames_host_check OK" when every expectation holds and the sanitizers stay silent.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>

#include "snn_c.h"

static int failures = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            ++failures;                                                \
            fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
        }                                                              \
    } while (0)

// the resolved line of a struct that lives in a heap block of exactly its size ("" = refused)
template <class T>
static std::string resolve(int entry, const T& io, int w = 32, int h = 24, int c = 1, int batch = 1) {
    std::unique_ptr<T> copy(new T(io));
    char buf[1024];
    return snn_frames_resolve(entry, copy.get(), w, h, c, batch, buf, sizeof(buf)) == 0 ? std::string(buf) : std::string();
}
static bool refusesNull(int entry) { return snn_frames_resolve(entry, nullptr, 32, 24, 1, 1, nullptr, 0) == -1; }
static std::string model(const std::string& line) { return line.substr(0, line.find(" | ")); }
static std::string planarTwin(std::string line) {
    const size_t at = line.find(" planar=0 | entry=");
    return at == std::string::npos ? std::string("?") : line.substr(0, at) + " planar=1 | entry=snn_model_create12";
}

static snn_frame_io2 io6(int fin, int fout, float mean, float norm, float scale, float offset, int in_shift = 0, int out_maxval = 65535, int out_shift = 0) {
    return snn_frame_io2{fin, fout, {mean, mean, mean, mean}, {norm, norm, norm, norm}, {scale, scale, scale, scale}, {offset, offset, offset, offset}, in_shift, out_maxval, out_shift};
}
static snn_frame_io io5(int fin, int fout, float mean, float norm, float scale, float offset) {
    return snn_frame_io{fin, fout, {mean, mean, mean, mean}, {norm, norm, norm, norm}, {scale, scale, scale, scale}, {offset, offset, offset, offset}};
}
// the luma maps include/snn_c.h states for snn_model_create9
static snn_video_io ranged(int format, int maxval, int shift, int siting, int range) {
    const double k = (maxval + 1) / 256.0, off = range == SNN_RANGE_LIMITED ? 16.0 * k : 0.0, span = range == SNN_RANGE_LIMITED ? 219.0 * k : maxval;
    return snn_video_io{format, maxval, shift, siting, static_cast<float>(off), static_cast<float>(1.0 / span), static_cast<float>(span), static_cast<float>(off)};
}

int main() {
    // ---- "built exactly as"
    const std::string floatModel = model(resolve(5, io5(0, 0, 0, 1, 1, 0)));
    EXPECT(!floatModel.empty() && snn_frames_resolve(5, nullptr, 32, 24, 1, 1, nullptr, 0) == 0 && snn_frames_resolve(6, nullptr, 32, 24, 1, 1, nullptr, 0) == 0);
    for (int fmt : {int(SNN_IO_RGB8), int(SNN_IO_RGBA8)}) { // create7 = create5 with R8 at both ends and the same maps
        const snn_colour_io c{fmt, 0.2126f, 0.0722f, 16.0f, 1.0f / 219.0f, 219.0f, 16.0f};
        EXPECT(model(resolve(7, c)) == model(resolve(5, io5(SNN_IO_R8, SNN_IO_R8, 16.0f, 1.0f / 219.0f, 219.0f, 16.0f))));
        EXPECT(resolve(7, c).find("source=rgb sink=rgb_merged") != std::string::npos);
    }
    for (int siting : {int(SNN_SITING_CENTRE), int(SNN_SITING_LEFT)})
        for (int range : {int(SNN_RANGE_LIMITED), int(SNN_RANGE_FULL)}) {
            struct Depth {
                int nv, planar, maxval, shift, rgb, rgba;
            };
            for (const Depth& d : {Depth{SNN_IO_NV12, SNN_IO_I420, 255, 0, SNN_IO_RGB8, SNN_IO_RGBA8}, Depth{SNN_IO_NV12_16, SNN_IO_I420_16, 1023, 6, SNN_IO_RGB16, SNN_IO_RGBA16},
                                   Depth{SNN_IO_NV12_16, SNN_IO_I420_16, 1023, 0, SNN_IO_RGB16, SNN_IO_RGBA16}, Depth{SNN_IO_NV12_16, SNN_IO_I420_16, 4095, 0, SNN_IO_RGB16, SNN_IO_RGBA16}}) {
                const snn_video_io v = ranged(d.nv, d.maxval, d.shift, siting, range);
                const std::string line8 = resolve(8, v);
                // create8 = create5 with R8 (NV12), create6 with R16, in_shift = out_shift = shift, out_maxval = maxval (NV12_16)
                EXPECT(!line8.empty() && model(line8) == model(d.nv == SNN_IO_NV12 ? resolve(5, io5(SNN_IO_R8, SNN_IO_R8, v.in_mean, v.in_norm, v.out_scale, v.out_offset))
                                                                                  : resolve(6, io6(SNN_IO_R16, SNN_IO_R16, v.in_mean, v.in_norm, v.out_scale, v.out_offset, d.shift, d.maxval, d.shift))));
                const snn_fit_io f{v, 48, 36}; // create11 = create8
                EXPECT(model(resolve(11, f)) == model(line8) && resolve(11, f).find("sink=fitted") != std::string::npos && resolve(11, f).find("fit=48x36") != std::string::npos);
                for (int out : {d.rgb, d.rgba}) { // create9 = create8 with the range's maps
                    const snn_video_rgb_io r{d.nv, out, d.maxval, d.shift, siting, range, 0.2126f, 0.0722f};
                    EXPECT(model(resolve(9, r)) == model(line8) && resolve(9, r).find("sink=rgb_from_yuv") != std::string::npos);
                    const snn_planar_io p{d.planar, out, d.maxval, d.shift, siting, range, 0.2126f, 0.0722f, 0, 0};
                    EXPECT(resolve(12, p) == planarTwin(resolve(9, r)));
                }
                const snn_planar_io same{d.planar, d.planar, d.maxval, d.shift, siting, range, 0.0f, 2.0f, 0, 0}; // (planar to planar: the matrix is not looked at)
                EXPECT(resolve(12, same) == planarTwin(line8));
                snn_planar_io fitted = same;
                fitted.out_w = 48, fitted.out_h = 36;
                EXPECT(resolve(12, fitted) == planarTwin(resolve(11, f)));
            }
            for (int fmt : {int(SNN_IO_RGB8), int(SNN_IO_RGBA8)}) { // create10 = create5 with R8, mean 0, norm 1/255 and the range's scale / offset; the extent may be odd
                const snn_encode_io e{fmt, SNN_IO_NV12, siting, range, 0.299f, 0.114f};
                const bool limited = range == SNN_RANGE_LIMITED;
                EXPECT(model(resolve(10, e, 31, 23)) == model(resolve(5, io5(SNN_IO_R8, SNN_IO_R8, 0.0f, 1.0f / 255.0f, limited ? 219.0f : 255.0f, limited ? 16.0f : 0.0f))));
                const snn_planar_io p{fmt, SNN_IO_I420, 255, 0, siting, range, 0.299f, 0.114f, 0, 0};
                EXPECT(resolve(12, p) == planarTwin(resolve(10, e)));
            }
        }

    // ---- refusals: null structs, the model input's own numbers, each entry point's rules
    for (int entry : {7, 8, 9, 10, 11, 12}) EXPECT(refusesNull(entry));
    for (int entry : {4, 13, 0, -1}) EXPECT(snn_frames_resolve(entry, nullptr, 32, 24, 1, 1, nullptr, 0) == -1);
    for (int entry = 5; entry <= 6; ++entry)
        EXPECT(snn_frames_resolve(entry, nullptr, 0, 24, 1, 1, nullptr, 0) == -1 && snn_frames_resolve(entry, nullptr, 32, -1, 1, 1, nullptr, 0) == -1 &&
               snn_frames_resolve(entry, nullptr, 32, 24, 0, 1, nullptr, 0) == -1 && snn_frames_resolve(entry, nullptr, 32, 24, 1, 0, nullptr, 0) == -1);
    for (const snn_frame_io& io : {io5(SNN_IO_R16, SNN_IO_R8, 0, 1, 1, 0), io5(SNN_IO_R8, SNN_IO_R16, 0, 1, 1, 0), io5(2, SNN_IO_R8, 0, 1, 1, 0), io5(SNN_IO_R8, 5, 0, 1, 1, 0),
                                   io5(SNN_IO_RGB8, SNN_IO_RGB8, 0, 1, 1, 0), io5(SNN_IO_NV12, SNN_IO_NV12, 0, 1, 1, 0)}) // the 8-bit formats only; RGB8 on a one-channel model
        EXPECT(resolve(5, io).empty());
    EXPECT(!resolve(5, io5(SNN_IO_RGB8, SNN_IO_RGB8, 0, 1, 1, 0), 32, 24, 3).empty());
    for (const snn_frame_io2& io : {io6(SNN_IO_R16, SNN_IO_R16, 0, 1, 1, 0, -1, 1023, 0), io6(SNN_IO_R16, SNN_IO_R16, 0, 1, 1, 0, 16, 1023, 0), io6(SNN_IO_R16, SNN_IO_R16, 0, 1, 1, 0, 0, 0, 0),
                                    io6(SNN_IO_R16, SNN_IO_R16, 0, 1, 1, 0, 0, 65536, 0), io6(SNN_IO_R16, SNN_IO_R16, 0, 1, 1, 0, 0, 1023, -1), io6(SNN_IO_R16, SNN_IO_R16, 0, 1, 1, 0, 0, 1023, 16),
                                    io6(SNN_IO_R16, SNN_IO_R16, 0, 1, 1, 0, 0, 1023, 7), io6(SNN_IO_RGB16, SNN_IO_RGB16, 0, 1, 1, 0, 0, 1023, 0), io6(2, SNN_IO_R16, 0, 1, 1, 0, 0, 1023, 0)})
        EXPECT(resolve(6, io).empty());
    EXPECT(!resolve(6, io6(SNN_IO_R8, SNN_IO_R16, 0, 1, 1, 0, 99, 65535, 0)).empty()); // the layout of an end that is not 16-bit is not looked at
    for (const snn_colour_io& io : {snn_colour_io{SNN_IO_R8, 0.299f, 0.114f, 0, 1, 1, 0}, snn_colour_io{SNN_IO_RGB16, 0.299f, 0.114f, 0, 1, 1, 0}, snn_colour_io{SNN_IO_RGB8, 0.0f, 0.114f, 0, 1, 1, 0},
                                    snn_colour_io{SNN_IO_RGB8, 0.299f, 0.0f, 0, 1, 1, 0}, snn_colour_io{SNN_IO_RGB8, 0.7f, 0.3f, 0, 1, 1, 0}})
        EXPECT(resolve(7, io).empty());
    const snn_colour_io colour{SNN_IO_RGB8, 0.299f, 0.114f, 0, 1, 1, 0};
    EXPECT(!resolve(7, colour, 31, 23).empty() && resolve(7, colour, 32, 24, 3).empty() && resolve(7, colour, 32, 24, 1, 0).empty());
    const snn_video_io nv12 = ranged(SNN_IO_NV12, 255, 0, SNN_SITING_LEFT, SNN_RANGE_LIMITED);
    EXPECT(resolve(8, nv12, 31, 24).empty() && resolve(8, nv12, 32, 23).empty() && resolve(8, nv12, 32, 24, 3).empty() && resolve(8, nv12, 32, 24, 1, 0).empty());
    for (const snn_video_io& io : {ranged(0, 255, 0, 1, 0), ranged(SNN_IO_R8, 255, 0, 1, 0), ranged(SNN_IO_R16, 255, 0, 1, 0), ranged(0x202, 255, 0, 1, 0), ranged(SNN_IO_NV12_16, 65535, 0, 1, 0),
                                   ranged(SNN_IO_NV12_16, 4096, 0, 1, 0), ranged(SNN_IO_NV12_16, 1023, 7, 1, 0), ranged(SNN_IO_NV12, 1023, 0, 1, 0), ranged(SNN_IO_NV12, 127, 1, 1, 0),
                                   ranged(SNN_IO_NV12, 255, 0, 2, 0), ranged(SNN_IO_NV12, 0, 0, 1, 0), ranged(SNN_IO_NV12_16, 1023, -1, 1, 0)}) {
        EXPECT(resolve(8, io).empty());
        EXPECT(resolve(11, snn_fit_io{io, 48, 36}).empty()); // create11 refuses what create8 refuses
    }
    for (const snn_fit_io& io : {snn_fit_io{nv12, 47, 36}, snn_fit_io{nv12, 48, 35}, snn_fit_io{nv12, 0, 36}, snn_fit_io{nv12, 48, 0}, snn_fit_io{nv12, 1, 1}, snn_fit_io{nv12, -2, 36},
                                 snn_fit_io{nv12, 48, -2}, snn_fit_io{nv12, 14, 36}, snn_fit_io{nv12, 130, 36}, snn_fit_io{nv12, 48, 10}, snn_fit_io{nv12, 48, 98}})
        EXPECT(resolve(11, io).empty());
    for (const snn_video_rgb_io& io : {snn_video_rgb_io{SNN_IO_R8, SNN_IO_RGB8, 255, 0, 1, 0, 0.299f, 0.114f}, snn_video_rgb_io{SNN_IO_NV12, SNN_IO_RGB16, 255, 0, 1, 0, 0.299f, 0.114f},
                                       snn_video_rgb_io{SNN_IO_NV12_16, SNN_IO_RGB8, 1023, 6, 1, 0, 0.299f, 0.114f}, snn_video_rgb_io{SNN_IO_NV12_16, SNN_IO_RGB16, 8191, 0, 1, 0, 0.299f, 0.114f},
                                       snn_video_rgb_io{SNN_IO_NV12_16, SNN_IO_RGB16, 1000, 0, 1, 0, 0.299f, 0.114f}, snn_video_rgb_io{SNN_IO_NV12, SNN_IO_RGB8, 127, 0, 1, 0, 0.299f, 0.114f},
                                       snn_video_rgb_io{SNN_IO_NV12, SNN_IO_RGB8, 255, 1, 1, 0, 0.299f, 0.114f}, snn_video_rgb_io{SNN_IO_NV12, SNN_IO_RGB8, 255, 0, 2, 0, 0.299f, 0.114f},
                                       snn_video_rgb_io{SNN_IO_NV12, SNN_IO_RGB8, 255, 0, 1, 2, 0.299f, 0.114f}, snn_video_rgb_io{SNN_IO_NV12, SNN_IO_RGB8, 255, 0, 1, 0, 0.0f, 0.114f},
                                       snn_video_rgb_io{SNN_IO_NV12, SNN_IO_RGB8, 255, 0, 1, 0, 0.7f, 0.3f}})
        EXPECT(resolve(9, io).empty());
    for (const snn_encode_io& io : {snn_encode_io{SNN_IO_R8, SNN_IO_NV12, 1, 0, 0.299f, 0.114f}, snn_encode_io{SNN_IO_RGB16, SNN_IO_NV12, 1, 0, 0.299f, 0.114f},
                                    snn_encode_io{SNN_IO_RGB8, SNN_IO_NV12_16, 1, 0, 0.299f, 0.114f}, snn_encode_io{SNN_IO_RGB8, SNN_IO_NV12, 2, 0, 0.299f, 0.114f},
                                    snn_encode_io{SNN_IO_RGB8, SNN_IO_NV12, 1, -1, 0.299f, 0.114f}, snn_encode_io{SNN_IO_RGB8, SNN_IO_NV12, 1, 0, 0.299f, 0.0f}})
        EXPECT(resolve(10, io).empty());
    for (const snn_planar_io& io : {snn_planar_io{SNN_IO_NV12, SNN_IO_NV12, 255, 0, 1, 0, 0.299f, 0.114f, 0, 0}, snn_planar_io{SNN_IO_I420, SNN_IO_I420_16, 255, 0, 1, 0, 0.299f, 0.114f, 0, 0},
                                    snn_planar_io{SNN_IO_I420, SNN_IO_RGB16, 255, 0, 1, 0, 0.299f, 0.114f, 0, 0}, snn_planar_io{SNN_IO_RGB8, SNN_IO_NV12, 255, 0, 1, 0, 0.299f, 0.114f, 0, 0},
                                    snn_planar_io{SNN_IO_I420, SNN_IO_I420, 127, 0, 1, 0, 0.299f, 0.114f, 0, 0}, snn_planar_io{SNN_IO_I420_16, SNN_IO_I420_16, 1000, 0, 1, 0, 0.299f, 0.114f, 0, 0},
                                    snn_planar_io{SNN_IO_I420, SNN_IO_I420, 255, 0, 1, 2, 0.299f, 0.114f, 0, 0}, snn_planar_io{SNN_IO_I420, SNN_IO_RGB8, 255, 0, 1, 0, 0.0f, 0.114f, 0, 0},
                                    snn_planar_io{SNN_IO_I420, SNN_IO_RGB8, 255, 0, 1, 0, 0.299f, 0.114f, 48, 36}, snn_planar_io{SNN_IO_RGB8, SNN_IO_I420, 255, 0, 1, 0, 0.299f, 0.114f, 48, 36},
                                    snn_planar_io{SNN_IO_I420, SNN_IO_I420, 255, 0, 1, 0, 0.299f, 0.114f, 47, 36}, snn_planar_io{SNN_IO_I420, SNN_IO_I420, 255, 0, 1, 0, 0.299f, 0.114f, 130, 36}})
        EXPECT(resolve(12, io).empty());
    {
        char small[16]; // a short buffer is filled, terminated and not overrun
        memset(small, 0x7f, sizeof(small));
        EXPECT(snn_frames_resolve(5, nullptr, 32, 24, 1, 1, small, sizeof(small)) == 0 && strlen(small) == sizeof(small) - 1);
    }
    if (failures) {
        fprintf(stderr, "frames_host_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("frames_host_check OK\n");
    return 0;
}
