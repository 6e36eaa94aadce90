// deconv2d_mfma.hip -- Conv2DTranspose on the matrix cores: the s*s stride phases of a transposed convolution as implicit GEMMs over ONE staged tile of
// the low-resolution input.  Behind snnhip_deconv2d_plan_create (shape_ops.hip) for the shapes of deconv2d_mfma_eligible; DESIGN.md section 4.28.
//
// Arithmetic (include/snnhip.h): base = k - 1 - p; output row oy = s*py + r (py = position row, r = residue) meets kernel rows ky = c + s*t, t < T_c,
// c = (base - r) mod s, T_c = ceil((k - c) / s), at input rows py + d + t with d = (r - base + c) / s (an integer); zero outside the image.  Columns alike.
// Phase (ry, rx) is a T_c(ry) x T_c(rx) stride-1 correlation whose GEMM is D[oc][position] += W_phase[oc][(ty, tx, ic)] * X[(ty, tx, ic)][position];
// the phases' tap counts sum to k*k (k % s != 0 gives phases of different depth: the loops run to each phase's own counts, no zero taps).
//
// Block = 256 threads = 4 waves = a tile of TH x 16 positions, all s*s phases of it (s*TH x 16*s output pixels), 16*NB output channels (the grid walks OC first).
//   s = 1: TH = 16, the one phase's rows split over the waves (4 rows each)        s = 2: TH = 8, one phase per wave
//   s = 3: TH = 4, phases w, w + 4, w + 8 of wave w (3 / 2 / 2 / 2)               s = 4: TH = 2, four phases per wave
// NB = 2 (s = 1 and OC > 32: 4): at most 96 accumulator registers per lane -- the 128-register forms (s = 2 with NB = 4, s = 4 with TH = 4) spilled
// to scratch at two waves per SIMD and are not built.  The channel chunk is the fastest block index, so the chunks of one tile run side by side and
// all but the first stage their input from L2.
// A wave's unit is (phase, G tile rows): G pixel groups of 16 positions (one tile row each = the MFMA's N) x NB row blocks of 16 channels (M) = G * NB
// independent accumulator chains per unit, all of a wave's units live over the whole K loop, so the input is staged once per IC chunk for all phases.
//
// Input: per IC chunk of 64 bytes (16 floats / 32 halfs) the halo tile (TH + ext) x (16 + ext) positions, ext = hi - lo of the d + t range (= ceil(k/s)
// when s divides k), 16-byte loads, zero-filled outside the image and beyond IC.  LDS pixel = 64 B = four 16-byte slots; lane (px = lane & 15,
// kq = lane >> 4) reads slot kq of position px shifted by the tap with one ds_read_b128: the operand of 4 fp32 K-steps (channels 4 kq + j) or of one
// 16x16x32 f16 MFMA (channels 8 kq .. + 7).  Slot swizzle slot' = slot ^ (((col >> 2) & 1) << 1), the 64-byte-pixel map of espcn_f16_wide.hip: a
// ds_read_b128 is served in lane groups of eight lanes of an even kq (pixels {0-3, 12-15}) and eight of kq + 1 (pixels {4-11}); bit 0 of the slot keeps
// the two kq apart, and two pixels of one residue mod 4 inside either set are 12 resp. 4 columns apart, so bit 0 of col >> 2 differs: 16 distinct
// 16-byte bank units for every tap shift.  Staging writes whole slots through the same map.
//
// Weights: packed once on the host into the A-operand image [phase][row block][tap][IC chunk][lane] x 16 bytes and read per K-step from L2 straight
// into the operand registers (conv2d_ksplit's way; the image of a 4x4 128 -> 64 layer is 512 KB).  Row m of block b is channel 32 (b >> 1) + 8 (m >> 2)
// + 4 (b & 1) + (m & 3), so a lane's accumulators of a block pair are eight consecutive channels: the epilogue stores straight from the accumulator
// layout, 2 x 16 B (fp32) or 16 B (fp16) per lane, the four kq of a pixel side by side.  Ragged IC / OC are zero rows / columns of the image, ragged OC
// masked at the store; tensor bases are 64-bit.
// IC no multiple of 4 (fp32) / 8 (fp16) or OC no multiple of 4: pixels are not 16-byte aligned, staging loads and stores go element by element
// (outside the K loop, which is the same).
#include "deconv2d_mfma.h"
#include "epilogue.h"
#include "plan_util.h"

namespace snnhip {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kTW = 16; // positions per tile row = the MFMA's N

struct DeconvMfmaArgs {
    int N, H, W, IC, OC, OH, OW;
    int tilesX, tilesY, ocChunks;
    int lo;        // input coordinate of halo row / column 0, relative to the tile's first position
    int HC;        // halo columns (kTW + ext); the rows are TH + ext
    int halo;      // ext
    int nch;       // IC chunks of 64 bytes
    int act, useBN;
    float leaky;
    int off[4];    // per residue r: d(r) - lo
    int nt[4];     // per residue r: T_c(r)
    int wbase[16]; // per phase ry * s + rx: where its image starts, in 16-byte units
};

template <typename T>
__device__ __forceinline__ void mfma_step(const uint4& a, const uint4& b, f32x4& acc) {
    if (sizeof(T) == 2) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
    } else {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, a.x), __builtin_bit_cast(float, b.x), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, a.y), __builtin_bit_cast(float, b.y), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, a.z), __builtin_bit_cast(float, b.z), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, a.w), __builtin_bit_cast(float, b.w), acc, 0, 0, 0);
    }
}

__device__ __forceinline__ int halo_slot(int slot, int col) { return slot ^ (((col >> 2) & 1) << 1); }

template <typename T, int S, int TH, int NB>
__global__ __launch_bounds__(256) void deconv2d_mfma_kernel(DeconvMfmaArgs a, const T* __restrict__ x, const uint4* __restrict__ wimg,
                                                           const float4* __restrict__ epi, T* __restrict__ y) {
    constexpr int RS = S == 1 ? 4 : 1;            // row splits of a phase
    constexpr int G = TH / RS;                    // pixel groups (tile rows) of a unit
    constexpr int UNITS = S * S * RS;
    constexpr int U = (UNITS + 3) / 4;            // units of a wave
    constexpr int ICC = 64 / static_cast<int>(sizeof(T)); // channels of an IC chunk
    static_assert(NB % 2 == 0 && TH % RS == 0, "row blocks come in pairs");
    extern __shared__ uint4 smem[];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, px = lane & 15, kq = lane >> 4;
    int bx = blockIdx.x;
    const int ocb0 = (bx % a.ocChunks) * NB;
    bx /= a.ocChunks;
    const int tx = bx % a.tilesX;
    bx /= a.tilesX;
    const int ty = bx % a.tilesY, n = bx / a.tilesY;
    const int py0 = ty * TH, px0 = tx * kTW;
    const int haloSlots = (TH + a.halo) * a.HC * 4;
    const T* xn = x + static_cast<size_t>(n) * a.H * a.W * a.IC;
    const bool vecIn = (a.IC * static_cast<int>(sizeof(T))) % 16 == 0;

    f32x4 acc[U][G][NB];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[u][g][nb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    for (int ch = 0; ch < a.nch; ++ch) {
        if (ch) __syncthreads();
        for (int idx = threadIdx.x; idx < haloSlots; idx += 256) {
            const int pos = idx >> 2, slot = idx & 3, hr = pos / a.HC, hc = pos - hr * a.HC;
            const int iy = py0 + a.lo + hr, ix = px0 + a.lo + hc, ic = ch * ICC + slot * (ICC / 4);
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W && ic < a.IC) {
                const T* src = xn + (static_cast<size_t>(iy) * a.W + ix) * a.IC + ic;
                if (vecIn) {
                    v = *reinterpret_cast<const uint4*>(src);
                } else { // a pixel is no whole number of 16-byte slots: element loads, zeros beyond IC
                    T e[ICC / 4];
#pragma unroll
                    for (int j = 0; j < ICC / 4; ++j) e[j] = ic + j < a.IC ? src[j] : static_cast<T>(0.0f);
                    __builtin_memcpy(&v, e, 16);
                }
            }
            smem[pos * 4 + halo_slot(slot, hc)] = v;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int unit = wave + 4 * u;
            if (unit < UNITS) {
                const int ph = unit / RS, row0 = (unit % RS) * G, ry = ph / S, rx = ph % S;
                const int nty = a.nt[ry], ntx = a.nt[rx], ntaps = nty * ntx;
                const uint4* wu = wimg + a.wbase[ph] + lane;
                for (int t = 0; t < ntaps; ++t) {
                    const int tyy = t / ntx, txx = t - tyy * ntx;
                    const int hc = px + a.off[rx] + txx;
                    const uint4* lb = smem + ((row0 + a.off[ry] + tyy) * a.HC + hc) * 4 + halo_slot(kq, hc);
                    uint4 av[NB], bv[G];
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) av[nb] = wu[(static_cast<size_t>((ocb0 + nb) * ntaps + t) * a.nch + ch) * 64];
#pragma unroll
                    for (int g = 0; g < G; ++g) bv[g] = lb[g * a.HC * 4];
#pragma unroll
                    for (int g = 0; g < G; ++g)
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb) mfma_step<T>(av[nb], bv[g], acc[u][g][nb]);
                }
            }
        }
    }

    // epilogue: lane (px, kq) holds channels 16 (ocb0 + nb) + 8 kq .. + 7 of a block pair (nb, nb + 1) at position px of each of its groups
    const bool vec8 = (a.OC & 7) == 0, vec4 = (a.OC & 3) == 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int unit = wave + 4 * u;
        if (unit < UNITS) {
            const int ph = unit / RS, row0 = (unit % RS) * G, ry = ph / S, rx = ph % S;
            const int ox = S * (px0 + px) + rx;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int oy = S * (py0 + row0 + g) + ry;
                if (oy < a.OH && ox < a.OW) {
                    T* dst = y + ((static_cast<size_t>(n) * a.OH + oy) * a.OW + ox) * a.OC;
#pragma unroll
                    for (int nb = 0; nb < NB; nb += 2) {
                        const int oc = 16 * (ocb0 + nb) + 8 * kq;
                        float lo4[4], hi4[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            lo4[i] = epi_act(a.act, a.leaky, epi_affine(acc[u][g][nb][i], epi[oc + i], a.useBN), 0.0f);
                            hi4[i] = epi_act(a.act, a.leaky, epi_affine(acc[u][g][nb + 1][i], epi[oc + 4 + i], a.useBN), 0.0f);
                        }
                        if (sizeof(T) == 2 && vec8) {
                            const float o8[8] = {lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
                            if (oc < a.OC) stv<T, 8>(dst + oc, o8);
                        } else if (vec4) {
                            if (oc < a.OC) stv<T, 4>(dst + oc, lo4);
                            if (oc + 4 < a.OC) stv<T, 4>(dst + oc + 4, hi4);
                        } else { // OC no multiple of 4: a pixel's channels are not 16-byte aligned, element stores
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                if (oc + i < a.OC) dst[oc + i] = static_cast<T>(lo4[i]);
                                if (oc + 4 + i < a.OC) dst[oc + 4 + i] = static_cast<T>(hi4[i]);
                            }
                        }
                    }
                }
            }
        }
    }
}

// tile rows / row blocks per stride: see the header comment
int tile_rows(int s) { return s == 1 ? 16 : s == 2 ? 8 : s == 3 ? 4 : 2; }
int row_blocks(int s, int OC) { return (s == 1 && OC > 32) ? 4 : 2; }

// Everything the plan derives from the layer before it owns anything: the tile, the phases (per residue r of the output coordinate its first kernel
// row c, tap count T_c and first input row d relative to the position), the grid and the sizes of the two weight images.
struct DeconvMfmaCfg {
    int TH = 0, NB = 0, nblk = 0, ldsBytes = 0;
    int c[4] = {0, 0, 0, 0};
    int nch[2] = {0, 0};       // IC chunks, [0] fp32 (16 channels), [1] fp16 (32)
    size_t lanes[2] = {0, 0};  // 16-byte units of either image
    DeconvMfmaArgs a;          // everything but nch / wbase, which depend on the element type
};

// false: not a shape of this kernel (the entry point keeps deconv2d_direct)
bool resolve(const DeconvGeom& g, DeconvMfmaCfg* cfg) {
    const int s = g.s, k = g.k;
    if (!(s >= 1 && s <= 4 && k >= 1 && up_div(k, s) <= 5 && g.IC >= 16 && g.OC >= 16 && g.OH <= s * g.H + k - s && g.OW <= s * g.W + k - s)) return false;
    cfg->TH = tile_rows(s);
    cfg->NB = row_blocks(s, g.OC);
    cfg->nblk = round_up(up_div(g.OC, 16), cfg->NB);
    DeconvMfmaArgs& a = cfg->a;
    memset(&a, 0, sizeof(a));
    const int base = k - 1 - g.p;
    int d[4] = {0, 0, 0, 0}, lo = 1 << 30, hi = -(1 << 30);
    for (int r = 0; r < s; ++r) {
        cfg->c[r] = ((base - r) % s + s) % s;
        a.nt[r] = cfg->c[r] < k ? up_div(k - cfg->c[r], s) : 0; // k < s: a residue no kernel row meets (bias only)
        d[r] = (r - base + cfg->c[r]) / s;                       // exact: the numerator is a multiple of s
        lo = std::min(lo, d[r]);
    }
    for (int r = 0; r < s; ++r) hi = std::max(hi, std::max(lo, d[r] + a.nt[r] - 1));
    for (int r = 0; r < s; ++r) a.off[r] = d[r] - lo;
    a.N = g.N; a.H = g.H; a.W = g.W; a.IC = g.IC; a.OC = g.OC; a.OH = g.OH; a.OW = g.OW;
    a.tilesY = up_div(up_div(g.OH, s), cfg->TH);
    a.tilesX = up_div(up_div(g.OW, s), kTW);
    a.ocChunks = cfg->nblk / cfg->NB;
    a.lo = lo;
    a.halo = hi - lo;
    a.HC = kTW + a.halo;
    a.act = g.act; a.useBN = g.useBN; a.leaky = g.leaky;
    cfg->ldsBytes = (cfg->TH + a.halo) * a.HC * 64;
    for (int f16 = 0; f16 < 2; ++f16) {
        cfg->nch[f16] = up_div(g.IC, f16 ? 32 : 16);
        cfg->lanes[f16] = static_cast<size_t>(cfg->nblk) * k * k * cfg->nch[f16] * 64; // the phases' tap counts sum to k*k
    }
    // the limits of the kernel's 32-bit indices and of a block's LDS
    return cfg->ldsBytes <= 64 * 1024 && static_cast<double>(a.tilesX) * a.tilesY * g.N * a.ocChunks < 2147483647.0 && cfg->lanes[0] < (1u << 30);
}

struct DeconvMfmaPlan : snnhip_plan {
    DeconvGeom g;
    DeconvMfmaCfg cfg;
    int wbaseOf[2][16];
    float* d_w[2] = {nullptr, nullptr};
    float* d_epi = nullptr;
    int described = -1;

    // the description and `bytes` name the element type of the last run (fp32 until a run has happened: the layer's type comes with its tensors)
    void describe(int f16) {
        if (described == f16) return;
        described = f16;
        const double es = f16 ? 2.0 : 4.0;
        bytes = es * (static_cast<double>(g.N) * g.H * g.W * g.IC + static_cast<double>(g.N) * g.OH * g.OW * g.OC) + 16.0 * static_cast<double>(cfg.lanes[f16]);
        char buf[256];
        snprintf(buf, sizeof(buf), "deconv2d_mfma_%s k=%d s=%d p=%d ic=%d oc=%d tile=%dx%d phases=%d x %doc chunk=%d lds=%dB %dx%d->%dx%d",
                 f16 ? "f16_16x16x32" : "f32_16x16x4", g.k, g.s, g.p, g.IC, g.OC, cfg.TH, kTW, g.s * g.s, 16 * cfg.NB, f16 ? 32 : 16, cfg.ldsBytes, g.H, g.W, g.OH,
                 g.OW);
        desc = buf;
    }

    template <typename T>
    int launch(const DeconvMfmaArgs& a, dim3 grid, const snnhip_tensor* in, snnhip_tensor* out) {
        const uint4* w = reinterpret_cast<const uint4*>(d_w[sizeof(T) == 2 ? 1 : 0]);
        const float4* e = reinterpret_cast<const float4*>(d_epi);
#define SNNHIP_DECONV_CASE(S_, TH_, NB_)                                                                                                           \
    if (g.s == S_ && cfg.TH == TH_ && cfg.NB == NB_) {                                                                                             \
        SNNHIP_LAUNCH((deconv2d_mfma_kernel<T, S_, TH_, NB_>), grid, dim3(256), static_cast<size_t>(cfg.ldsBytes), ctx->stream, a, cptr<T>(in), w, e, \
                      mptr<T>(out));                                                                                                              \
        return SNNHIP_OK;                                                                                                                          \
    }
        SNNHIP_DECONV_CASE(1, 16, 2)
        SNNHIP_DECONV_CASE(1, 16, 4)
        SNNHIP_DECONV_CASE(2, 8, 2)
        SNNHIP_DECONV_CASE(3, 4, 2)
        SNNHIP_DECONV_CASE(4, 2, 2)
#undef SNNHIP_DECONV_CASE
        SNNHIP_REQUIRE(false, "deconv2d_mfma: no kernel instance for s=%d tile rows=%d row blocks=%d", g.s, cfg.TH, cfg.NB);
    }

    int run(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) override {
        SNNHIP_REQUIRE(nIn == 1, "deconv2d: expects 1 input, got %d", nIn);
        SNNHIP_SAME_DTYPE("deconv2d");
        SNNHIP_REQUIRE(out->dtype == SNNHIP_F32 || out->dtype == SNNHIP_F16, "deconv2d: tensor dtype %d", out->dtype);
        SNNHIP_REQUIRE(dims_match(in[0], g.N, g.H, g.W, g.IC) && dims_match(out, g.N, g.OH, g.OW, g.OC), "deconv2d: tensor dims do not match the plan (%s)",
                       desc.c_str());
        const int f16 = out->dtype == SNNHIP_F16 ? 1 : 0;
        describe(f16);
        DeconvMfmaArgs a = cfg.a;
        a.nch = cfg.nch[f16];
        memcpy(a.wbase, wbaseOf[f16], sizeof(a.wbase));
        const dim3 grid(static_cast<unsigned>(a.tilesX) * a.tilesY * g.N * a.ocChunks);
        const int rc = f16 ? launch<_Float16>(a, grid, in[0], out) : launch<float>(a, grid, in[0], out);
        if (rc != SNNHIP_OK) return rc;
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }
};

} // namespace

bool deconv2d_mfma_eligible(const DeconvGeom& g) {
    DeconvMfmaCfg cfg;
    return resolve(g, &cfg);
}

int make_deconv2d_mfma_plan(snnhip_ctx* ctx, const DeconvGeom& g, const float* w_oihw, const std::vector<float>& epi4, snnhip_plan** out) {
    DeconvMfmaCfg cfg;
    SNNHIP_REQUIRE(resolve(g, &cfg), "deconv2d_mfma: k=%d s=%d ic=%d oc=%d is not a shape of this kernel", g.k, g.s, g.IC, g.OC);
    SNNHIP_REQUIRE(static_cast<int>(epi4.size()) >= cfg.nblk * 16 * 4, "deconv2d_mfma: epilogue table of %zu floats for %d row blocks", epi4.size(), cfg.nblk);
    auto* plan = new DeconvMfmaPlan(); // nothing below returns without handing the plan over or deleting it
    plan->ctx = ctx;
    plan->anyDtype = true;
    plan->g = g;
    plan->cfg = cfg;
    const int s = g.s, k = g.k;

    // the A-operand images, one per element type: [phase][row block][tap][IC chunk][lane] x 16 bytes
    int rc = SNNHIP_OK;
    for (int f16 = 0; f16 < 2 && rc == SNNHIP_OK; ++f16) {
        const int icc = f16 ? 32 : 16, per = icc / 4, nch = cfg.nch[f16];
        std::vector<float> img(cfg.lanes[f16] * 4, 0.0f);
        _Float16* imgh = reinterpret_cast<_Float16*>(img.data());
        size_t at = 0;
        for (int ry = 0; ry < s; ++ry)
            for (int rx = 0; rx < s; ++rx) {
                plan->wbaseOf[f16][ry * s + rx] = static_cast<int>(at);
                const int nty = cfg.a.nt[ry], ntx = cfg.a.nt[rx];
                for (int b = 0; b < cfg.nblk; ++b)
                    for (int t = 0; t < nty * ntx; ++t) {
                        const int ky = cfg.c[ry] + s * (t / ntx), kx = cfg.c[rx] + s * (t % ntx);
                        for (int ch = 0; ch < nch; ++ch)
                            for (int lane = 0; lane < 64; ++lane, ++at) {
                                const int m = lane & 15, kq = lane >> 4, oc = 32 * (b >> 1) + 8 * (m >> 2) + 4 * (b & 1) + (m & 3);
                                if (oc >= g.OC) continue;
                                for (int j = 0; j < per; ++j) {
                                    const int ic = ch * icc + kq * per + j;
                                    if (ic >= g.IC) break;
                                    const float wv = w_oihw[((static_cast<size_t>(oc) * g.IC + ic) * k + ky) * k + kx];
                                    if (f16)
                                        imgh[at * 8 + j] = static_cast<_Float16>(wv); // the conversion of conv2d_mfma's fp16 packer
                                    else
                                        img[at * 4 + j] = wv;
                                }
                            }
                    }
            }
        rc = plan->upload(img.data(), img.size(), &plan->d_w[f16]);
    }
    if (rc == SNNHIP_OK) rc = plan->upload(epi4.data(), epi4.size(), &plan->d_epi);
    if (rc != SNNHIP_OK) {
        delete plan;
        return rc;
    }
    for (int i = 0; i < 4; ++i) {
        plan->inDims[i] = (i == 0 ? g.N : i == 1 ? g.H : i == 2 ? g.W : g.IC);
        plan->outDims[i] = (i == 0 ? g.N : i == 1 ? g.OH : i == 2 ? g.OW : g.OC);
    }
    plan->flops = 2.0 * g.N * g.H * g.W * k * k * static_cast<double>(g.IC) * g.OC;
    plan->describe(0);
    *out = plan;
    return SNNHIP_OK;
}

} // namespace snnhip
