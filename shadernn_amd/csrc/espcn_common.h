// espcn_common.h -- what the ESPCN kernel units (espcn_fused.hip, espcn_d2s_mfma.hip, espcn_f16.hip, espcn_f16_wide.hip) and the chain planner share:
// the tile order, the kernels' frame-end parameter blocks and the host-side description of a frame end (FrameIn / FrameOut).
#pragma once
#include <hip/hip_runtime.h>

namespace snnhip {

// XCD-aware tile order (guide T1): workgroup b runs on XCD b % 8 and every XCD has a private 4 MiB L2.  Handing each XCD
// a contiguous run of tiles keeps the halo rows/columns that neighbouring tiles share inside one L2 instead of
// re-fetching them through the fabric.  Bijective for any grid size; purely a performance hint.
__device__ __forceinline__ int xcd_tile_order(int b, int nb) {
    const int q = nb >> 3, r = nb & 7;
    const int xcd = b & 7, k = b >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

// Chain rule A8: an 8-bit input frame normalised while the tile is staged, y = (float(u) - mean) * norm (snnhip_u8_in_plan_create's map)
struct U8InCfg {
    float mean, norm;
};
// Chain rule B8: the output frame quantised in the epilogue, q = quantize_u8(o, scale, offset) (snnhip_u8_out_plan_create's map)
struct U8OutCfg {
    float scale, offset;
};
// The 16-bit forms of the two (snnhip_u16_in_plan_create's / snnhip_u16_out_plan_create's maps) carry parameter blocks of their own, so that the
// blocks of the 8-bit kernels stay what they are: y = (float(u >> shift) - mean) * norm;  q = quantize_u16(o, scale, offset, maxval) << shift
struct U16InCfg {
    float mean, norm;
    int shift;
};
struct U16OutCfg {
    float scale, offset, maxval;
    int shift;
};
// What a fused kernel's frame end stores: 0 = the launch's own tensor type (float / _Float16), 8 / 16 = an 8- / 16-bit frame.  (A 16-bit frame
// element and a half are both 2 bytes: the kernel bodies ask this trait, not sizeof.)
template <typename T>
struct FrameBits {
    static constexpr int value = 0;
};
template <>
struct FrameBits<unsigned char> {
    static constexpr int value = 8;
};
template <>
struct FrameBits<unsigned short> {
    static constexpr int value = 16;
};

// ---- host side: the one description of a frame end that the planner hands to a launch function.  bits as FrameBits: 0 = the launch reads / writes its
// own tensor type, 8 / 16 = a frame (the maps of snnhip_u8_in / u16_in and snnhip_u8_out / u16_out; shift and maxval are the 16-bit forms').  Never a
// kernel argument: each launch function builds its kernel's own block from it (U8InCfg{f.mean, f.norm}, ...), and which block a kernel keeps its 8-bit
// map in is its unit's matter.
struct FrameIn {
    int bits = 0;
    float mean = 0.0f, norm = 1.0f;
    int shift = 0;
};
struct FrameOut {
    int bits = 0;
    float scale = 1.0f, offset = 0.0f, maxval = 0.0f;
    int shift = 0;
};

// MFMA row of a depth-to-space tail (kernel B for r = 3 / 4, kernel B16): row 4*dy + dx holds channel r*dy + dx (r = 2, 3, 4); -1 = the row stays zero
inline int espcn_d2s_row_channel(int r, int row) { return ((row & 3) < r && (row >> 2) < r) ? r * (row >> 2) + (row & 3) : -1; }

} // namespace snnhip
