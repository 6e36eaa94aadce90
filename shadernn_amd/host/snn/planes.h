// planes.h -- rows between pitched planes in the caller's memory and a dense buffer (snn_model_upload_frame_planes / _download_frame_planes,
// include/snn_c.h).  HIP extension: the reference has no video frame path.  Header-only so that tools/planar_host_check.cpp runs it under a sanitizer
// without a device.
#pragma once
#include <cstddef>
#include <cstring>

namespace snn {

// true when the pieces (each `rows` rows of `rowBytes` bytes, pitch[i] bytes apart) are tight and follow one another in memory: one dense run
inline bool planesAreDense(char* const* pieces, const size_t* pitch, size_t nPieces, size_t rowBytes, size_t rows) {
    for (size_t i = 0; i < nPieces; ++i)
        if (pitch[i] != rowBytes || pieces[i] != pieces[0] + i * rowBytes * rows) return false;
    return true;
}

// piece i, row y <-> dense + (i * rows + y) * rowBytes.  Exactly rowBytes bytes of every row are read (toDense) or written: never the padding
inline void copyPlaneRows(char* dense, char* const* pieces, const size_t* pitch, size_t nPieces, size_t rowBytes, size_t rows, bool toDense) {
    for (size_t i = 0; i < nPieces; ++i)
        for (size_t y = 0; y < rows; ++y) {
            char* host = pieces[i] + y * pitch[i];
            char* d = dense + (i * rows + y) * rowBytes;
            if (toDense) memcpy(d, host, rowBytes);
            else memcpy(host, d, rowBytes);
        }
}

} // namespace snn
