// frame_resample.h -- the one definition of what the frame kernels around the luma model share (frame_colour.hip, frame_chroma.hip,
// frame_yuv_rgb.hip, frame_rgb_cbcr.hip): the Keys cubic and its phase, the tap-table filler behind the four
// snnhip_bicubic_taps* entry points, the five-weight form of a table, the matrix and sample-format checks of the plan descs, the r x C launch dispatch,
// and on the device the quantiser, the element of a run of dwords, loads and stores of dword-aligned runs, the five-weight horizontal filter and the
// tile decode.  Which bytes a lane loads and stores and its geometry stay with each unit.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "../../include/snnhip.h"
#include "snnhip_internal.h"

namespace snnhip {

// ---- host: the filter

// Keys cubic convolution kernel, a = -0.5 (Catmull-Rom), at distance d >= 0; plain products in double, no contraction, so that the same expression in
// any IEEE double arithmetic gives the same bits
inline double keys_cubic(double d) {
#pragma clang fp contract(off)
    const double a = -0.5;
    if (d <= 1.0) return (a + 2.0) * (d * d * d) - (a + 3.0) * (d * d) + 1.0;
    if (d < 2.0) return a * (d * d * d) - 5.0 * a * (d * d) + 8.0 * a * d - 4.0 * a;
    return 0.0;
}

// The phase: output sample R*x + p of an R-fold resampling reads source position x + s, s = (p + lead) / R - off.  `lead` is where the output sample
// sits inside its own cell, `off` where the source sample sits inside its cell, both in units of the cell.  base = floor(s), taps at
// x + base - 1 .. x + base + 2 with the Keys weights at distances 1 + t, t, 1 - t, 2 - t, t = s - base.
// ... and, for a grid whose step is not one source cell per R outputs, output sample p of a pattern that advances `step` / `den` source cells per output:
// s = (step * p + lead) / den - off (bicubic_phase_general is step = 1, den = R)
inline void bicubic_phase_ratio(int step, int den, int p, double lead, double off, int* base, double w[4]) {
#pragma clang fp contract(off)
    const double s = (step * p + lead) / den - off;
    const double i0 = std::floor(s);
    const double t = s - i0;
    *base = static_cast<int>(i0);
    w[0] = keys_cubic(1.0 + t);
    w[1] = keys_cubic(t);
    w[2] = keys_cubic(1.0 - t);
    w[3] = keys_cubic(2.0 - t);
}
inline void bicubic_phase_general(int R, int p, double lead, double off, int* base, double w[4]) { bicubic_phase_ratio(1, R, p, lead, off, base, w); }

inline bool siting_ok(int siting) { return siting == SNNHIP_SITING_CENTRE || siting == SNNHIP_SITING_LEFT; }
// where a chroma sample sits inside its cell: co-sited with the even luma column (left) or between the two (centre)
inline double siting_offset(int siting) { return siting == SNNHIP_SITING_LEFT ? 0.25 : 0.5; }

// aligned pixel centres: sx = (X + 0.5) / r - 0.5 = x + (p + 0.5) / r - 0.5
inline void bicubic_phase(int r, int p, int* first, double w[4]) { bicubic_phase_general(r, p, 0.5, 0.5, first, w); }
// the output is itself a chroma grid of the same siting: s = (p + off) / r - off
inline void bicubic_phase_sited(int r, int p, int siting, int* base, double w[4]) {
    bicubic_phase_general(r, p, siting_offset(siting), siting_offset(siting), base, w);
}
// A 4:2:0 chroma plane resampled straight to the OUTPUT LUMA grid, R = 2r-fold: output luma column X = R*x + p sits at low-resolution luma position
// (X + 0.5) / r - 0.5, which halved is chroma index (X + 0.5) / R - 0.25 for left-sited chroma (sample i co-sited with luma column 2i) and
// (X + 0.5) / R - 0.5 for centred chroma: lead = 0.5 either way.
inline void bicubic_phase_420(int R, int p, int siting, int* base, double w[4]) { bicubic_phase_general(R, p, 0.5, siting_offset(siting), base, w); }

// The table behind snnhip_bicubic_taps / _sited / _420 / _rgb420 (`name` without the prefix): `phases` rows of four float weights and each row's base,
// for a `phases`-fold resampling with (lead, off); `r` is the caller's upscale factor, the one the messages speak of.  The first three advance one
// source cell per `phases` outputs and know bases -1 and 0 only; _rgb420 advances `step` / `den` cells per output (bicubic_phase_ratio) and reaches
// base `maxBase` = 1.
inline int fill_bicubic_taps(const char* name, int r, int phases, int siting, double lead, double off, float* weights, int* base, int capacity, int step = 1, int den = 0,
                             int maxBase = 0) {
    SNNHIP_REQUIRE(weights && base, "%s: null argument", name);
    SNNHIP_REQUIRE(r >= 1 && r <= 4, "%s: r = %d (1..4)", name, r);
    SNNHIP_REQUIRE(siting_ok(siting), "%s: siting %d (SNNHIP_SITING_CENTRE or SNNHIP_SITING_LEFT)", name, siting);
    SNNHIP_REQUIRE(capacity >= 4 * phases, "%s: room for %d floats, %d needed", name, capacity, 4 * phases);
    for (int p = 0; p < phases; ++p) {
        double w[4];
        int b = 0;
        bicubic_phase_ratio(step, den ? den : phases, p, lead, off, &b, w);
        SNNHIP_REQUIRE(b >= -1 && b <= maxBase, "%s: phase %d of r = %d starts at %d", name, p, r, b);
        base[p] = b;
        for (int k = 0; k < 4; ++k) weights[4 * p + k] = static_cast<float>(w[k]);
    }
    return SNNHIP_OK;
}

// a phase's four weights at base - 1 .. base + 2 as five weights over -2 .. 2 (w5 zeroed by the caller): the base is folded into the table, so that
// a kernel indexes its registers with compile-time constants (a term 0 * v adds exactly nothing)
template <int ROWS>
inline void widen_taps(int phases, const float* w4, const int* base, float (&w5)[ROWS][5]) {
    for (int p = 0; p < phases; ++p)
        for (int k = 0; k < 4; ++k) w5[p][base[p] + 1 + k] = w4[4 * p + k];
}

// ---- host: what the plan descs share

inline bool matrix_ok(float kr, float kb) { return kr > 0.0f && kb > 0.0f && kr + kb < 1.0f; }

// The sample format of a video desc: 8-bit samples or 16-bit containers holding `maxval` << `shift`, chroma sited.  `what` starts every message
// ("chroma_up desc"), `unit` is what the desc calls its 8-bit images ("planes", "frames"); *bits is the container's width.
inline int check_sample_format(const char* what, const char* unit, int dtype, int siting, int shift, int maxval, int* bits) {
    SNNHIP_REQUIRE(dtype == SNNHIP_U8 || dtype == SNNHIP_U16, "%s: dtype %d (SNNHIP_U8 or SNNHIP_U16)", what, dtype);
    SNNHIP_REQUIRE(siting_ok(siting), "%s: siting %d (SNNHIP_SITING_CENTRE or SNNHIP_SITING_LEFT)", what, siting);
    const int b = dtype == SNNHIP_U8 ? 8 : 16;
    SNNHIP_REQUIRE(shift >= 0 && shift < b && (b == 16 || shift == 0), "%s: shift %d (0 for 8-bit %s, 0..15 for 16-bit containers)", what, shift, unit);
    SNNHIP_REQUIRE(maxval >= 1, "%s: maxval %d (at least 1)", what, maxval);
    // the fp32 filter on full 16-bit values is 1.5e-2 away from its float64 value: too far for a rounding contract (P016 is not built)
    SNNHIP_REQUIRE(maxval <= 4095, "%s: maxval %d is above 4095 (12 bits): the fp32 filter cannot keep the rounding contract for wider samples", what, maxval);
    SNNHIP_REQUIRE((static_cast<long long>(maxval) << shift) < (1ll << b), "%s: maxval %d << shift %d does not fit %d bits", what, maxval, shift, b);
    *bits = b;
    return SNNHIP_OK;
}

// f(R, C) with R = std::integral_constant<int, r> and C = std::integral_constant<int, c>, for r in 1..4 and c one of C0, C1 (both checked when the
// plan was made): the one place where a desc's (r, channels) picks a kernel instance
template <int C0, int C1, typename F>
inline void dispatch_r_c(int r, int c, F&& f) {
    auto with_r = [&](auto R) {
        if (c == C0) f(R, std::integral_constant<int, C0>{});
        else f(R, std::integral_constant<int, C1>{});
    };
    switch (r) {
    case 1: with_r(std::integral_constant<int, 1>{}); break;
    case 2: with_r(std::integral_constant<int, 2>{}); break;
    case 3: with_r(std::integral_constant<int, 3>{}); break;
    default: with_r(std::integral_constant<int, 4>{}); break;
    }
}

// ---- device

// clamp(rint(v), 0, maxval), ties to even, NaN -> 0
__device__ __forceinline__ unsigned quantize_frame(float v, float maxval) {
    v = rintf(v);
    v = v >= 0.0f ? v : 0.0f; // NaN fails the test: 0
    v = v <= maxval ? v : maxval;
    return static_cast<unsigned>(v);
}

// element i of a run of E (8- or 16-bit) held as dwords
template <typename E>
__device__ __forceinline__ unsigned frame_elem(const unsigned* w, int i) {
    constexpr int PER = 4 / static_cast<int>(sizeof(E)), BITS = 8 * static_cast<int>(sizeof(E));
    return (w[i / PER] >> (BITS * (i % PER))) & ((1u << BITS) - 1u);
}

// NW (1..4) dwords at an address that is only dword-aligned, as one access: a vector type whose alignment is lowered to 4, which global memory
// takes at any width
template <int NW>
struct WordsOf;
template <>
struct WordsOf<1> {
    typedef unsigned type __attribute__((aligned(4)));
};
template <>
struct WordsOf<2> {
    typedef unsigned type __attribute__((ext_vector_type(2), aligned(4)));
};
template <>
struct WordsOf<3> {
    typedef unsigned type __attribute__((ext_vector_type(3), aligned(4)));
};
template <>
struct WordsOf<4> {
    typedef unsigned type __attribute__((ext_vector_type(4), aligned(4)));
};
template <int NW>
__device__ __forceinline__ void load_words(const void* p, unsigned* w) {
    if constexpr (NW == 1) {
        w[0] = *reinterpret_cast<const unsigned*>(p);
    } else {
        const typename WordsOf<NW>::type q = *reinterpret_cast<const typename WordsOf<NW>::type*>(p);
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = q[k];
    }
}
// NW dwords (any number) to a dword-aligned address, four at a time
template <int NW>
__device__ __forceinline__ void store_words(void* p, const unsigned* w) {
    if constexpr (NW > 4) {
        store_words<4>(p, w);
        store_words<NW - 4>(reinterpret_cast<unsigned*>(p) + 4, w + 4);
    } else if constexpr (NW == 1) {
        *reinterpret_cast<unsigned*>(p) = w[0];
    } else {
        typename WordsOf<NW>::type q;
#pragma unroll
        for (int k = 0; k < NW; ++k) q[k] = w[k];
        *reinterpret_cast<typename WordsOf<NW>::type*>(p) = q;
    }
}

// One staged row v (PX + 4 pixels of C channels: two pixels of apron either side) to the lane's PHASES * PX output pixels: output pixel j reads
// input pixel j / PHASES at phase j % PHASES, five weights over its offsets -2 .. 2
template <int PHASES, int C, int PX, int ROWS>
__device__ __forceinline__ void frame_hfilter(const float (&w)[ROWS][5], const float* v, float* h) {
    static_assert(PHASES <= ROWS, "the table has a row for every phase");
#pragma unroll
    for (int j = 0; j < PHASES * PX; ++j) {
        const int x = j / PHASES, p = j % PHASES;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float acc = w[p][0] * v[x * C + c];
#pragma unroll
            for (int k = 1; k < 5; ++k) acc += w[p][k] * v[(x + k) * C + c];
            h[j * C + c] = acc;
        }
    }
}

// block b of a grid of N * tilesY * tilesX tiles, x fastest
struct FrameTile {
    int tx, ty;
    size_t n;
};
__device__ __forceinline__ FrameTile frame_tile(unsigned b, int tilesX, int tilesY) {
    FrameTile t;
    t.tx = static_cast<int>(b % static_cast<unsigned>(tilesX));
    t.ty = static_cast<int>((b / static_cast<unsigned>(tilesX)) % static_cast<unsigned>(tilesY));
    t.n = b / (static_cast<unsigned>(tilesX) * static_cast<unsigned>(tilesY));
    return t;
}

} // namespace snnhip
