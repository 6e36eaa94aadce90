// planar_host_check.cpp -- the host paths of the planar-frame feature that need no device, as a stand-alone program for a sanitizer build (DESIGN.md
// section 4.19): every refusal of snn_model_create12 that returns before a model file is opened (what depends on the model's r -- r = 1 with RGB in,
// a fitted size outside [r * in / 2, r * in] -- needs a device context and is tests/test_frame_planar_host_gpu.py's), the refusals of the plane
// functions that need no model, and the row gather / scatter between pitched planes and a dense buffer (shadernn_amd/host/snn/planes.h) on heap
// blocks of exactly the planes' size, so that a byte read or written past a row's end or in the padding of the last row is an error the sanitizer
// reports.  Built against lib/libsnn_core_asan.so (python -c "import __graft_entry__ as g; g.build_host(sanitize='address,undefined')"):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Iinclude -Ishadernn_amd/host tools/planar_host_check.cpp -o build/planar_host_check \
//       -Lshadernn_amd/lib -lsnn_core_asan -lsnnhip -Wl,-rpath,$PWD/shadernn_amd/lib -Wl,-rpath,/opt/rocm/lib
// Exit status 0 and "planar_host_check OK" when every expectation holds and the sanitizers stay silent.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <utility>
#include <vector>

#include "snn/planes.h"
#include "snn_c.h"

static int failures = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            ++failures;                                                \
            fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
        }                                                              \
    } while (0)

static snn_planar_io planar(int in_format = SNN_IO_I420, int out_format = SNN_IO_I420, int maxval = 255, int shift = 0, int siting = SNN_SITING_LEFT,
                            int range = SNN_RANGE_LIMITED, float kr = 0.299f, float kb = 0.114f, int out_w = 0, int out_h = 0) {
    snn_planar_io io{};
    io.in_format = in_format;
    io.out_format = out_format;
    io.maxval = maxval;
    io.shift = shift;
    io.siting = siting;
    io.range = range;
    io.kr = kr;
    io.kb = kb;
    io.out_w = out_w;
    io.out_h = out_h;
    return io;
}

static int create12(const snn_planar_io* io, int w = 32, int h = 24, int in_c = 1, int batch = 1) {
    snn_model* m = nullptr;
    const int rc = snn_model_create12("no/such/model.json", 0, w, h, in_c, 0, 1, 0, 0, 0, batch, io, &m);
    EXPECT(m == nullptr);
    return rc;
}

int main() {
    static_assert(sizeof(snn_planar_io) == 40, "snn_planar_io is 10 * 4 bytes");
    const int I8 = SNN_IO_I420, I16 = SNN_IO_I420_16;

    // snn_model_create12: everything it refuses before the model file is opened
    EXPECT(create12(nullptr) == -1);
    const snn_planar_io good = planar();
    EXPECT(create12(&good, 31, 24) == -1 && create12(&good, 32, 23) == -1 && create12(&good, 0, 24) == -1 && create12(&good, 32, 0) == -1); // odd or empty extents
    EXPECT(create12(&good, 32, 24, 3) == -1 && create12(&good, 32, 24, 1, 0) == -1 && create12(&good, 32, 24, 1, -1) == -1);                 // channels and batch
    for (const snn_planar_io& io : {
             // formats that do not pair up
             planar(0, I8), planar(SNN_IO_R8, I8), planar(SNN_IO_NV12, SNN_IO_NV12), planar(SNN_IO_NV12, I8), planar(I8, SNN_IO_NV12), planar(I8, I16, 255), planar(I16, I8, 1023),
             planar(I8, SNN_IO_RGB16), planar(I8, SNN_IO_RGBA16), planar(I16, SNN_IO_RGB8, 1023), planar(I16, SNN_IO_RGBA8, 1023), planar(I8, SNN_IO_R8), planar(I8, 0),
             planar(SNN_IO_RGB8, SNN_IO_NV12), planar(SNN_IO_RGB8, I16), planar(SNN_IO_RGB8, SNN_IO_RGB8), planar(SNN_IO_RGB16, I16, 1023), planar(SNN_IO_RGB16, I8),
             // depth, shift
             planar(I8, I8, 256), planar(I8, I8, 0), planar(I8, I8, 127), planar(I8, I8, 1023), planar(I8, I8, 255, 1), planar(I8, I8, 255, -1), planar(I16, I16, 65535),
             planar(I16, I16, 8191), planar(I16, I16, 1000), planar(I16, I16, 254), planar(I16, I16, 1023, 7), planar(I16, I16, 1023, 16), planar(I16, I16, 4095, 5),
             planar(I8, SNN_IO_RGB8, 127), planar(I16, SNN_IO_RGB16, 1000), planar(I16, SNN_IO_RGB16, 1023, 7),
             // siting, range on every path
             planar(I8, I8, 255, 0, 2), planar(I8, I8, 255, 0, -1), planar(I8, I8, 255, 0, SNN_SITING_LEFT, 2), planar(I8, I8, 255, 0, SNN_SITING_LEFT, -1),
             planar(I8, SNN_IO_RGB8, 255, 0, 2), planar(I8, SNN_IO_RGB8, 255, 0, SNN_SITING_LEFT, 2), planar(SNN_IO_RGB8, I8, 255, 0, 2),
             planar(SNN_IO_RGB8, I8, 255, 0, SNN_SITING_LEFT, 2),
             // the matrix of an RGB end
             planar(I8, SNN_IO_RGB8, 255, 0, 1, 0, 0.0f), planar(I8, SNN_IO_RGB8, 255, 0, 1, 0, 0.299f, -0.1f), planar(I8, SNN_IO_RGBA8, 255, 0, 1, 0, 0.7f, 0.3f),
             planar(SNN_IO_RGB8, I8, 255, 0, 1, 0, 0.0f), planar(SNN_IO_RGBA8, I8, 255, 0, 1, 0, 0.7f, 0.3f),
             // a fitted size together with an RGB end
             planar(I8, SNN_IO_RGB8, 255, 0, 1, 0, 0.299f, 0.114f, 48, 36), planar(I16, SNN_IO_RGB16, 1023, 0, 1, 0, 0.299f, 0.114f, 48, 36),
             planar(SNN_IO_RGB8, I8, 255, 0, 1, 0, 0.299f, 0.114f, 48, 36), planar(I8, SNN_IO_RGB8, 255, 0, 1, 0, 0.299f, 0.114f, 48, 0),
             // the fitted size's own rules: even, at least 2, out / in within [1/2, 4]
             planar(I8, I8, 255, 0, 1, 0, 0.299f, 0.114f, 47, 36), planar(I8, I8, 255, 0, 1, 0, 0.299f, 0.114f, 48, 35), planar(I8, I8, 255, 0, 1, 0, 0.299f, 0.114f, 48, 0),
             planar(I8, I8, 255, 0, 1, 0, 0.299f, 0.114f, 0, 36), planar(I8, I8, 255, 0, 1, 0, 0.299f, 0.114f, -2, 36), planar(I8, I8, 255, 0, 1, 0, 0.299f, 0.114f, 14, 36),
             planar(I8, I8, 255, 0, 1, 0, 0.299f, 0.114f, 130, 36), planar(I8, I8, 255, 0, 1, 0, 0.299f, 0.114f, 48, 10), planar(I16, I16, 1023, 0, 1, 0, 0.299f, 0.114f, 48, 98)})
        EXPECT(create12(&io) == -1);

    // the plane functions without a model or without arguments
    {
        unsigned char y[4] = {0}, cb[1] = {0}, cr[1] = {0};
        const void* in[3] = {y, cb, cr};
        void* out[3] = {y, cb, cr};
        const int pitch[3] = {2, 1, 1};
        EXPECT(snn_model_upload_frame_planes(nullptr, in, pitch, 3) == -1);
        EXPECT(snn_model_download_frame_planes(nullptr, out, pitch, 3) == -1);
        EXPECT(snn_model_upload_frame_planes(nullptr, nullptr, pitch, 3) == -1);
        EXPECT(snn_model_download_frame_planes(nullptr, out, nullptr, 3) == -1);
    }

    // rows between pitched planes and a dense buffer.  Every plane is a heap block that ENDS with its last row's last byte (no padding behind the last
    // row, as a cropped view of a surface has none): one byte too many, read or written, is out of bounds
    for (size_t es : {size_t(1), size_t(2)})
        for (size_t width : {size_t(1), size_t(7), size_t(16)})
            for (size_t pad : {size_t(0), size_t(13)}) {
                const size_t rows = 5, nPieces = 4, rowBytes = width * es, pitchBytes = rowBytes + pad;
                const size_t block = (rows - 1) * pitchBytes + rowBytes;
                std::vector<char*> pieces;
                std::vector<size_t> pitch(nPieces, pitchBytes);
                for (size_t i = 0; i < nPieces; ++i) {
                    char* p = new char[block];
                    memset(p, 0xA5, block);
                    for (size_t yy = 0; yy < rows; ++yy)
                        for (size_t x = 0; x < rowBytes; ++x) p[yy * pitchBytes + x] = static_cast<char>(1 + (i * 31 + yy * 7 + x) % 100);
                    pieces.push_back(p);
                }
                EXPECT(!snn::planesAreDense(pieces.data(), pitch.data(), nPieces, rowBytes, rows)); // separate heap blocks never follow one another
                char* dense = new char[nPieces * rows * rowBytes];
                snn::copyPlaneRows(dense, pieces.data(), pitch.data(), nPieces, rowBytes, rows, true);
                for (size_t i = 0; i < nPieces; ++i)
                    for (size_t yy = 0; yy < rows; ++yy)
                        for (size_t x = 0; x < rowBytes; ++x) EXPECT(dense[(i * rows + yy) * rowBytes + x] == static_cast<char>(1 + (i * 31 + yy * 7 + x) % 100));
                for (size_t k = 0; k < nPieces * rows * rowBytes; ++k) dense[k] = static_cast<char>(dense[k] + 100);
                snn::copyPlaneRows(dense, pieces.data(), pitch.data(), nPieces, rowBytes, rows, false);
                for (size_t i = 0; i < nPieces; ++i)
                    for (size_t yy = 0; yy < rows; ++yy)
                        for (size_t x = 0; x < pitchBytes && yy * pitchBytes + x < block; ++x) {
                            const char want = x < rowBytes ? static_cast<char>(101 + (i * 31 + yy * 7 + x) % 100) : static_cast<char>(0xA5); // the padding is untouched
                            EXPECT(pieces[i][yy * pitchBytes + x] == want);
                        }
                // tight planes cut from one block, in order, are one dense run; out of order they are not
                std::vector<char*> cut;
                std::vector<size_t> tight(nPieces, rowBytes);
                for (size_t i = 0; i < nPieces; ++i) cut.push_back(dense + i * rows * rowBytes);
                EXPECT(snn::planesAreDense(cut.data(), tight.data(), nPieces, rowBytes, rows));
                std::swap(cut[1], cut[2]);
                EXPECT(!snn::planesAreDense(cut.data(), tight.data(), nPieces, rowBytes, rows));
                for (char* p : pieces) delete[] p;
                delete[] dense;
            }
    if (failures) {
        fprintf(stderr, "planar_host_check: %d expectation(s) failed\n", failures);
        return 1;
    }
    printf("planar_host_check OK\n");
    return 0;
}
