// frame_fit_core.h -- the two-pass fit that plane_fit (frame_fit.hip) and rgb_fit (frame_rgb_fit.hip) share: the table of
// one axis, the tables of a plan and the checks the kernels rely on, the tile geometry, the vertical pass into LDS and what a lane of the horizontal
// pass keeps in registers.  A unit supplies its rule for the table, its strips (FitTile, a strip policy) and the epilogue of its horizontal pass.
// The Keys cubic, the siting check and the block-to-tile map are frame_resample.h's.
#pragma once
#include <vector>

#include "frame_resample.h"

namespace snnhip {

constexpr int kFitTaps = 8; // Keys values per output coordinate before any are dropped: taps at base - 3 .. base + 4

// What tells the axis tables of the units apart.  Output X of `out` reads source position Nn / D of `in` samples, Nn = (4X + lead) in - a out,
// D = 4 out, a = 4 * the siting's offset (1: left, 2: centre): lead = a when the output grid is sited as the input is, 2 when it is a luma grid.
struct FitRule {
    bool sitedLead;     // the numerator's lead is a (else 2)
    bool stretch;       // f = min(out / in, 1): the kernel widens when the axis shrinks (else f = 1)
    int shrink, grow;   // the admitted ratios: in / shrink <= out <= grow * in ...
    const char* window; // ... as the refusal prints them
    int k0, nk;         // the taps a table row keeps: k0 .. k0 + nk - 1 of the eight
};

// The table of one axis: row X holds the kept weights of output X and base[X] = floor(Nn / D); t = (Nn - base D) / D.  Tap k sits at base - 3 + k,
// its weight is the Keys cubic at |k - 3 - t| * f; the eight are summed in ascending order in double, each divided by the sum and rounded to float.
inline int fill_fit_taps(const FitRule& R, const char* name, int in, int out, int siting, float* weights, int* base, int capacity) {
#pragma clang fp contract(off)
    SNNHIP_REQUIRE(weights && base, "%s: null argument", name);
    SNNHIP_REQUIRE(in >= 1 && out >= 1, "%s: %d -> %d samples (both at least 1)", name, in, out);
    SNNHIP_REQUIRE(siting_ok(siting), "%s: siting %d (SNNHIP_SITING_CENTRE or SNNHIP_SITING_LEFT)", name, siting);
    SNNHIP_REQUIRE(static_cast<long long>(R.shrink) * out >= in && out <= static_cast<long long>(R.grow) * in, "%s: %d -> %d samples is a ratio outside %s", name, in, out,
                   R.window);
    SNNHIP_REQUIRE(static_cast<long long>(capacity) >= static_cast<long long>(R.nk) * out, "%s: room for %d floats, %lld needed", name, capacity,
                   static_cast<long long>(R.nk) * out);
    const long long a = siting == SNNHIP_SITING_LEFT ? 1 : 2;
    const long long lead = R.sitedLead ? a : 2;
    const long long D = 4ll * out;
    const double f = R.stretch && out < in ? static_cast<double>(out) / static_cast<double>(in) : 1.0;
    for (int X = 0; X < out; ++X) {
        const long long Nn = (4ll * X + lead) * in - a * out;
        long long b = Nn / D;
        if (Nn % D < 0) --b; // floor
        const double t = static_cast<double>(Nn - b * D) / static_cast<double>(D);
        double w[kFitTaps], sum = 0.0;
        for (int k = 0; k < kFitTaps; ++k) {
            w[k] = keys_cubic(std::fabs(static_cast<double>(k - 3) - t) * f);
            sum += w[k];
        }
        base[X] = static_cast<int>(b);
        for (int k = 0; k < R.nk; ++k) weights[static_cast<size_t>(R.nk) * X + k] = static_cast<float>(w[R.k0 + k] / sum);
    }
    return SNNHIP_OK;
}

// ---- geometry.  A block of 256 threads owns an output tile of TH x TW pixels: TW one output dword per lane of a wave, TH what the 48 KB of LDS
// hold of vertically filtered float rows over the tile's input column span.  The span is cut into strips, what one lane loads of an input row.
constexpr int kFitThreads = 256;
constexpr int kFitWaves = kFitThreads / 64;
constexpr int kFitLdsFloats = 12288; // 48 KB of static LDS: three blocks per CU
constexpr int kFitMaxRows = 32;      // output rows per tile at most
constexpr int kFitAhead = 4;         // rows a strip's loads run ahead of their use
// rows of floats are skewed by one float every 32: lanes that start 4 or 8 floats apart (a dword of outputs at ratio 1 or 1/2) then fall on 32
// different banks of a ds_read_b32 instead of 8 or 4
__host__ __device__ constexpr int fit_skew(int i) { return i + (i >> 5); }

struct FitTile {
    int tw, stripFloats, maxStrips; // output pixels across, floats of a strip in a filtered row, strips of a tile's span at most
    constexpr int rowStride() const { return fit_skew(maxStrips * stripFloats - 1) + 1; } // floats
    constexpr int th() const { return kFitLdsFloats / rowStride() < kFitMaxRows ? kFitLdsFloats / rowStride() : kFitMaxRows; }
};

// What every fit kernel takes: the sizes, the quantiser and the four tables (device pointers).
struct FitHead {
    int N, H, W, OH, OW; // H, W: what is resampled
    int tilesX, tilesY;
    int shift;
    float maxval;
    const float* wy; // [OH][nk]
    const int* by;   // [OH]
    const float* wx; // [OW][nk]
    const int* bx;   // [OW]
};

// The tables of a plan on the host: built and checked, then uploaded into the plan's FitHead.
struct FitAxes {
    std::vector<float> wy, wx;
    std::vector<int> by, bx;
    int N = 0, H = 0, W = 0, tilesX = 0, tilesY = 0;

    // Both axes through the unit's entry point `taps` (rows are always centre-sited), then what the kernel relies on: bases never step back, and
    // no tile's column span -- the unit's geometry counts its strips from the bases of its first and last column -- has more strips than its
    // LDS rows hold.
    template <typename Geom>
    int build(const char* unit, int (*taps)(int, int, int, float*, int*, int), int nk, const Geom& g, int n, int h, int w, int OH, int OW, int siting) {
        const FitTile T = g.tile();
        N = n, H = h, W = w, tilesX = up_div(OW, T.tw), tilesY = up_div(OH, T.th());
        SNNHIP_REQUIRE(static_cast<double>(N) * tilesX * tilesY < 2147483648.0 && static_cast<double>(OW) * nk < 2.0e9 && static_cast<double>(OH) * nk < 2.0e9,
                       "%s desc: %dx%dx%d -> %dx%d is too large", unit, N, H, W, OH, OW);
        wy.resize(static_cast<size_t>(OH) * nk), wx.resize(static_cast<size_t>(OW) * nk);
        by.resize(OH), bx.resize(OW);
        int rc = taps(H, OH, SNNHIP_SITING_CENTRE, wy.data(), by.data(), static_cast<int>(wy.size()));
        if (rc == SNNHIP_OK) rc = taps(W, OW, siting, wx.data(), bx.data(), static_cast<int>(wx.size()));
        if (rc != SNNHIP_OK) return rc;
        for (int x = 1; x < OW; ++x) SNNHIP_REQUIRE(bx[x] >= bx[x - 1], "%s: column bases step back at %d", unit, x);
        for (int y = 1; y < OH; ++y) SNNHIP_REQUIRE(by[y] >= by[y - 1], "%s: row bases step back at %d", unit, y);
        for (int tx = 0; tx < tilesX; ++tx) {
            const int strips = g.strips(g.first(bx[tx * T.tw]), bx[std::min((tx + 1) * T.tw, OW) - 1]);
            SNNHIP_REQUIRE(strips <= T.maxStrips, "%s: tile column %d spans %d strips, %d fit", unit, tx, strips, T.maxStrips);
        }
        return SNNHIP_OK;
    }

    int upload(snnhip_plan* plan, FitHead* P, int shift, int maxval) const {
        *P = FitHead{N, H, W, static_cast<int>(by.size()), static_cast<int>(bx.size()), tilesX, tilesY, shift, static_cast<float>(maxval), nullptr, nullptr, nullptr, nullptr};
        int rc = upload_table(plan, wy, &P->wy);
        if (rc == SNNHIP_OK) rc = upload_table(plan, wx, &P->wx);
        if (rc == SNNHIP_OK) rc = upload_table(plan, by, &P->by);
        if (rc == SNNHIP_OK) rc = upload_table(plan, bx, &P->bx);
        return rc;
    }

    template <typename T>
    static int upload_table(snnhip_plan* plan, const std::vector<T>& v, const T** dev) {
        static_assert(sizeof(T) == sizeof(float), "the base tables travel through upload()"); // (a copy of bytes: ints are as wide as floats)
        float* d = nullptr;
        const int rc = plan->upload(reinterpret_cast<const float*>(v.data()), v.size(), &d);
        *dev = reinterpret_cast<const T*>(d);
        return rc;
    }
};

// The dword of elements e .. e + NE - 1 of a row of W pixels of C = 1 | 2 elements (what a strip of a plane is); `fast`: the row is dword-aligned
// and the strip lies inside it, otherwise elements with the pixel index clamped to [0, W - 1].
template <typename E, int C>
__device__ __forceinline__ unsigned fit_load_strip(const E* __restrict__ row, int e, int W, bool fast) {
    constexpr int NE = 4 / static_cast<int>(sizeof(E)), BITS = 8 * static_cast<int>(sizeof(E));
    unsigned w = 0u;
    if (fast) {
        load_words<1>(row + e, &w);
    } else {
#pragma unroll
        for (int j = 0; j < NE; ++j) {
            const int ee = e + j;
            const int px = min(max(ee >> (C - 1), 0), W - 1); // arithmetic shift: floor for the columns left of the plane
            w |= static_cast<unsigned>(row[static_cast<size_t>(px) * C + (ee & (C - 1))]) << (BITS * j);
        }
    }
    return w;
}

// ---- pass 1, vertical.  The tile's S strips walk down the input rows, a lane per strip, with a window of the last V::NT rows and raw loads
// kFitAhead rows ahead of their use, and write one filtered float row into lds per output row of the tile; the rows' bases and weights are the
// same for the whole block (scalar loads).  When S is below the block's size the tile's rows are dealt to as many lane sets as fit, each walking
// its own chunk (the chunks' halos are read again).  The strip policy V says what a strip is:
//   R, K0, NT        the unit's FitRule; the first tap read of the eight and how many
//   NR, NF           raw dwords of a strip in an input row; floats of a strip in a filtered row
//   Win, NW          a row of the window is NW values of type Win: the raw dwords, or what enter() made of them
//   pos(s)           where strip s starts in a row, in the unit's own measure;  fast(pos): whole dwords may be loaded there
//   load(cy, pos, fast, raw)   the raw dwords of input row cy, 0 <= cy < H
//   enter(raw, row)  a row enters the window;  at(row, j): float j of it, j < NF, as it is filtered
//   off(b)           (pass 2) the float of a filtered row at which the first tap read of a pixel with base b starts
// The order of every sum is fixed here: first product, then += in ascending k.
template <typename V>
__device__ __forceinline__ void fit_vertical_pass(const V& v, const FitHead& P, float* lds, int RS, int S, int oy0, int trows, int tid) {
    constexpr int NT = V::NT, K0 = V::K0, NR = V::NR, NF = V::NF, NW = V::NW;
    const int H = P.H;
    const int sets = S >= kFitThreads ? 1 : kFitThreads / S;
    const int chunk = (trows + sets - 1) / sets;
    for (int u = tid; u < S * sets; u += kFitThreads) {
        const int s = u % S, q = u / S;
        const int t0 = q * chunk, t1 = min(t0 + chunk, trows);
        if (t0 >= t1) continue;
        const auto pos = v.pos(s);
        const bool fast = v.fast(pos);
        int next = P.by[oy0 + t0] - 3 + K0;                    // the next input row to enter the window
        const int last = P.by[oy0 + t1 - 1] - 3 + K0 + NT - 1; // the last one this chunk reads
        typename V::Win win[NT][NW];
        unsigned pre[kFitAhead][NR];
#pragma unroll
        for (int k = 0; k < NT; ++k)
#pragma unroll
            for (int j = 0; j < NW; ++j) win[k][j] = 0;
#pragma unroll
        for (int k = 0; k < kFitAhead; ++k) v.load(min(max(min(next + k, last), 0), H - 1), pos, fast, pre[k]);
        for (int t = t0; t < t1; ++t) {
            const int top = P.by[oy0 + t] - 3 + K0 + NT; // one past the window's last row
            const float* wrow = P.wy + static_cast<size_t>(oy0 + t) * V::R.nk + (K0 - V::R.k0);
            while (next < top) {
#pragma unroll
                for (int k = 0; k + 1 < NT; ++k)
#pragma unroll
                    for (int j = 0; j < NW; ++j) win[k][j] = win[k + 1][j];
                v.enter(pre[0], win[NT - 1]);
#pragma unroll
                for (int k = 0; k + 1 < kFitAhead; ++k)
#pragma unroll
                    for (int j = 0; j < NR; ++j) pre[k][j] = pre[k + 1][j];
                v.load(min(max(min(next + kFitAhead, last), 0), H - 1), pos, fast, pre[kFitAhead - 1]);
                ++next;
            }
            float wk[NT];
#pragma unroll
            for (int k = 0; k < NT; ++k) wk[k] = wrow[k];
            float* dst = lds + t * RS;
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                float acc = wk[0] * v.at(win[0], j);
#pragma unroll
                for (int k = 1; k < NT; ++k) acc += wk[k] * v.at(win[k], j);
                dst[fit_skew(s * NF + j)] = acc;
            }
        }
    }
}

// ---- pass 2, horizontal: a wave covers the tile's width and takes every kFitWaves-th row, a lane (g = tid & 63) the NPX pixels X[p] of one output
// dword.  What the lane keeps in registers for all its rows: the weights of its pixels and off[p], the float of a filtered row at which the first
// tap read of pixel p starts (V's off(base)); valid, the pixels of its dword inside the frame.  A lane with g * NPX >= tcols has no dword in the
// tile: the kernel returns before it asks (the return has to be the kernel's own).
template <int NPX, int NT>
struct FitLane {
    int valid, X[NPX], off[NPX];
    float w[NPX][NT];
};
template <int NPX, typename V>
__device__ __forceinline__ FitLane<NPX, V::NT> fit_lane(const V& v, const FitHead& P, int g, int ox0, int tcols) {
    FitLane<NPX, V::NT> L;
#pragma unroll
    for (int p = 0; p < NPX; ++p) {
        const int X = min(ox0 + g * NPX + p, P.OW - 1);
        L.X[p] = X;
        L.off[p] = v.off(P.bx[X]);
#pragma unroll
        for (int k = 0; k < V::NT; ++k) L.w[p][k] = P.wx[static_cast<size_t>(X) * V::R.nk + (V::K0 - V::R.k0) + k];
    }
    L.valid = min(NPX, tcols - g * NPX);
    return L;
}

} // namespace snnhip
