// yolo_head.hip -- the YOLO v3 detection head on the device: decode, stable score sort and greedy NMS of one image in one block, one launch for the
// batch (include/snnhip.h: snnhip_yolo_head_plan_create / snnhip_plan_run_io).  The reference, and the host mirror's CPU stage,
// download both heads and walk them on the CPU (yololayer.cpp:27-226, host/layers.cpp: YOLOLayer::decode); this is the same list, row for row.
//
//   heads:  n_heads tensors T [N][g][g][A * (5 + classes)] (T = float or half), g = net_size / grid_scale[h]; candidate index = head, gy, gx, anchor.
//   out:    float [N][max_boxes][1][6] rows {class, score, x, y, w, h}, zeros past the count; float [N][1][1][2] = {rows written, boxes over the threshold}.
//
// One block of 256 threads per image; no scratch buffer, no global atomic, no memset: bit-identical from run to run, and recordable in a graph.
//   1. decode:  the threads stride over the M candidates; each finds the class (first maximum, strict >) and the confidence
//               1 / (1 + e^-obj (1 + e^-cls)).  A survivor takes a slot (wave ballot + mbcnt, one LDS counter per block, bumped once per wave) and
//               leaves a 64-bit key there: high word ~bits(score), low word candidate << 20 | class.  Ascending key order is the stable descending
//               score sort whatever order the slots were handed out in.
//   2. sort:    bitonic over the next power of two >= the survivor count (padding keys all-ones), one comparator per thread and pass.  Comparator c of
//               distance j owns elements i = c with a zero bit inserted at j and i | j, so the 64 comparators of a wave stay inside one aligned run of
//               128 keys for every j <= 32: those stages run back to back with a wave barrier only; a block barrier for j >= 64 and between merges.
//   3. boxes:   the box of every sorted position, computed once from its candidate's four geometry values, as float4 in LDS.
//   4. NMS:     one bit per sorted position in LDS.  Per kept box: wave 0 finds the next clear bit (a lane per 64-bit word, ballot + ffs) and
//               publishes it; all threads test the positions behind it (same class, yoloIoU > threshold); the 64 lanes of a wave cover one mask word, so
//               the update is a ballot ORed in by lane 0; thread 0 writes the row.  Two barriers per kept box; ends at max_boxes rows or the list's end.
// Arithmetic is fp32 with contraction off and IEEE division, expf from the device library: a decision can differ from the CPU's only through expf's
// last bits.  LDS per instance: CAP * (8 + 16) + CAP / 8 + 8 bytes, CAP = 256 / 1024 / 4096 candidates.
#include "plan_util.h"
#include "snnhip_internal.h"
#include "yolo_head.h"

namespace snnhip {
namespace {

struct YoloHeadParams {
    int nHeads, A, classes, vals; // vals = 5 + classes
    int grid[2];
    int first[3];                 // first candidate of head h; first[nHeads] = M
    float anchorW[2][kYoloHeadMaxAnchors], anchorH[2][kYoloHeadMaxAnchors]; // resolved through the masks
    float extent[2];              // float(grid_scale * grid)
    float conf, iou;
    int maxBoxes;
};

struct YoloBoxF {
    float x, y, w, h;
};

// yoloIoU (yololayer.cpp:57-72), in its operation order; std::max / std::min written out
__device__ __forceinline__ float yolo_iou(const YoloBoxF& a, const YoloBoxF& b) {
#pragma clang fp contract(off)
    const float x0 = a.x < b.x ? b.x : a.x, y0 = a.y < b.y ? b.y : a.y;
    const float ax1 = a.x + a.w, bx1 = b.x + b.w, ay1 = a.y + a.h, by1 = b.y + b.h;
    const float x1 = bx1 < ax1 ? bx1 : ax1, y1 = by1 < ay1 ? by1 : ay1;
    if (x1 < x0 || y1 < y0) return 0.0f;
    const float inter = (x1 - x0) * (y1 - y0);
    return inter / (a.w * a.h + b.w * b.h - inter);
}

__device__ __forceinline__ float yolo_sigmoid(float x) {
#pragma clang fp contract(off)
    return 1.0f / (1.0f + expf(-x));
}

// The values of one candidate: element i widened to float.  VEC: (5 + classes) * sizeof(T) is a multiple of 16 and the heads start on 16 bytes, so the
// 16-byte piece that holds element `anchor` (4: objectness, 0: geometry) is one load; everything outside it is read by elements.
template <typename T, bool VEC, int ANCHOR>
struct YoloVals {
    static constexpr int Q = 16 / static_cast<int>(sizeof(T)), piece = ANCHOR / Q;
    const T* p;
    float v[Q];
    __device__ __forceinline__ explicit YoloVals(const T* cand) : p(cand) {
        if constexpr (VEC) {
            const uint4 w = *reinterpret_cast<const uint4*>(cand + piece * Q);
            const unsigned u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int k = 0; k < Q; ++k) {
                if constexpr (sizeof(T) == 4) v[k] = __uint_as_float(u[k]);
                else v[k] = static_cast<float>(__builtin_bit_cast(_Float16, static_cast<unsigned short>((u[k / 2] >> (16 * (k % 2))) & 0xffffu)));
            }
        }
    }
    // element I (a constant, so that v[] stays in registers); an element outside the piece is read from memory
    template <int I>
    __device__ __forceinline__ float at() const {
        if constexpr (VEC && I / Q == piece) return v[I % Q];
        else return static_cast<float>(p[I]);
    }
};

struct YoloCand {
    int head, gx, gy, gc;
    size_t offset; // of the candidate's first value inside its image
};
__device__ __forceinline__ YoloCand yolo_candidate(const YoloHeadParams& P, int idx) {
    YoloCand c;
    c.head = (P.nHeads > 1 && idx >= P.first[1]) ? 1 : 0;
    const int local = idx - P.first[c.head];
    const int cell = local / P.A, g = P.grid[c.head];
    c.gc = local - cell * P.A;
    c.gy = cell / g;
    c.gx = cell - c.gy * g;
    c.offset = static_cast<size_t>(local) * P.vals;
    return c;
}

__device__ __forceinline__ void wave_sync_lds() { // LDS operations of a wave complete in order: only the compiler's order has to be kept
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void compare_exchange(unsigned long long* keys, int c, int j, int k) {
    const int i = ((c & ~(j - 1)) << 1) | (c & (j - 1)), l = i | j;
    const unsigned long long a = keys[i], b = keys[l];
    if ((a > b) == ((i & k) == 0)) keys[i] = b, keys[l] = a;
}

template <typename T, int CAP, bool VEC>
__global__ __launch_bounds__(kYoloHeadThreads) void yolo_head_kernel(YoloHeadParams P, const T* __restrict__ head0, const T* __restrict__ head1, float* __restrict__ rows,
                                                                      float* __restrict__ counts) {
#pragma clang fp contract(off)
    __shared__ unsigned long long keys[CAP];
    __shared__ float4 boxes[CAP];
    __shared__ unsigned long long merged[CAP / 64];
    __shared__ int survivors, nextKept;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t n = blockIdx.x;
    const int M = P.first[P.nHeads];
    const T* img[2] = {head0 + n * static_cast<size_t>(P.first[1] - P.first[0]) * P.vals,
                       P.nHeads > 1 ? head1 + n * static_cast<size_t>(P.first[2] - P.first[1]) * P.vals : head0};
    if (t == 0) survivors = 0;
    if (t < CAP / 64) merged[t] = 0;
    __syncthreads();

    // ---- 1. decode (yololayer.cpp:118-160)
    for (int base = 0; base < M; base += kYoloHeadThreads) { // (uniform trip count: the ballot below sees whole waves)
        const int idx = base + t;
        bool keep = false;
        unsigned long long key = 0;
        if (idx < M) {
            const YoloCand c = yolo_candidate(P, idx);
            const YoloVals<T, VEC, 4> v(img[c.head] + c.offset);
            int cls = 0;
            float maxLogit = -3.402823466e+38f;
            auto scan = [&](float x, int i) {
                if (x > maxLogit) maxLogit = x, cls = i - 5;
            };
            scan(v.template at<5>(), 5); // (vals >= 6; 6 and 7 sit in the objectness' piece when there is one)
            if (P.vals > 6) scan(v.template at<6>(), 6);
            if (P.vals > 7) scan(v.template at<7>(), 7);
            for (int i = 8; i < P.vals; ++i) scan(static_cast<float>(v.p[i]), i);
            const float prob = 1.0f / (1.0f + expf(-v.template at<4>()) * (1.0f + expf(-maxLogit)));
            keep = prob > P.conf;
            key = (static_cast<unsigned long long>(~__float_as_uint(prob)) << 32) | (static_cast<unsigned>(idx) << 20) | static_cast<unsigned>(cls);
        }
        const unsigned long long vote = __ballot(keep);
        if (vote) { // (wave-uniform)
            int slot0 = 0;
            if (lane == 0) slot0 = atomicAdd(&survivors, __popcll(vote)); // LDS
            slot0 = __shfl(slot0, 0);
            if (keep) keys[slot0 + static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(vote >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(vote), 0u)))] = key;
        }
    }
    __syncthreads();
    const int count = survivors;

    // ---- 2. sort: ascending keys = std::stable_sort by descending score (yololayer.cpp:213)
    int P2 = 2;
    while (P2 < count) P2 <<= 1;
    for (int i = count + t; i < P2; i += kYoloHeadThreads) keys[i] = ~0ull;
    __syncthreads();
    if (count > 1) {
        const int half = P2 >> 1;
        for (int k = 2; k <= P2; k <<= 1) {
            int j = k >> 1;
            for (; j >= 64; j >>= 1) {
                for (int c = t; c < half; c += kYoloHeadThreads) compare_exchange(keys, c, j, k);
                __syncthreads();
            }
            // A thread owns half / 256 comparators per stage (c = t, t + 256, ...).  For the tail it takes them one after the other and runs ALL the
            // remaining stages j <= 32 on one run of 128 keys, which only its own wave touches, before it moves to its next run.
            for (int c = t; c < half; c += kYoloHeadThreads)
                for (int jj = j; jj >= 1; jj >>= 1) {
                    compare_exchange(keys, c, jj, k);
                    wave_sync_lds();
                }
            if (k >= 64) __syncthreads(); // (merges up to 64 keys never leave the wave's run either)
        }
        __syncthreads();
    }

    // ---- 3. the box of every sorted position (yololayer.cpp:149-156)
    for (int p = t; p < count; p += kYoloHeadThreads) {
        const int idx = static_cast<int>(static_cast<unsigned>(keys[p]) >> 20);
        const YoloCand c = yolo_candidate(P, idx);
        const YoloVals<T, VEC, 0> v(img[c.head] + c.offset);
        const float g = static_cast<float>(P.grid[c.head]);
        const float cx = (static_cast<float>(c.gx) + yolo_sigmoid(v.template at<0>())) / g, cy = (static_cast<float>(c.gy) + yolo_sigmoid(v.template at<1>())) / g;
        const float w = expf(v.template at<2>()) * P.anchorW[c.head][c.gc] / P.extent[c.head];
        const float h = expf(v.template at<3>()) * P.anchorH[c.head][c.gc] / P.extent[c.head];
        boxes[p] = make_float4(cx - w / 2, cy - h / 2, w, h);
    }
    __syncthreads();

    // ---- 4. greedy NMS in sorted order (yololayer.cpp:74-112)
    float* out = rows + n * static_cast<size_t>(P.maxBoxes) * 6;
    const int words = (count + 63) >> 6;
    int kept = 0, from = 0;
    while (kept < P.maxBoxes && from < count) {
        if (wave == 0) { // lane l looks at mask word l (CAP / 64 <= 64 words)
            unsigned long long open = 0;
            if (lane < words) {
                open = ~merged[lane];
                if (lane == words - 1 && (count & 63)) open &= (1ull << (count & 63)) - 1;
                if (lane < (from >> 6)) open = 0;
                else if (lane == (from >> 6)) open &= ~0ull << (from & 63);
            }
            const unsigned long long any = __ballot(open != 0);
            const int bit = open ? __ffsll(static_cast<long long>(open)) - 1 : 0;
            const int word = any ? __ffsll(static_cast<long long>(any)) - 1 : 0;
            const int pos = (word << 6) + __shfl(bit, word);
            if (lane == 0) nextKept = any ? pos : -1;
        }
        __syncthreads();
        const int i = nextKept;
        if (i < 0) break; // (block-uniform)
        const unsigned long long ki = keys[i];
        const unsigned ci = static_cast<unsigned>(ki) & 0xfffffu;
        const float4 bi4 = boxes[i];
        const YoloBoxF bi = {bi4.x, bi4.y, bi4.z, bi4.w};
        if (t == 0) {
            float* r = out + static_cast<size_t>(kept) * 6;
            r[0] = static_cast<float>(ci);
            r[1] = __uint_as_float(~static_cast<unsigned>(ki >> 32));
            r[2] = bi.x, r[3] = bi.y, r[4] = bi.w, r[5] = bi.h;
        }
        ++kept;
        if (kept < P.maxBoxes) // (the rows past max_boxes are never asked for: nothing left to suppress)
            for (int w = ((i + 1) >> 6) + wave; w < words; w += kYoloHeadThreads / 64) {
                const int j = (w << 6) + lane;
                bool hit = false;
                if (j > i && j < count && (static_cast<unsigned>(keys[j]) & 0xfffffu) == ci) {
                    const float4 bj4 = boxes[j];
                    const YoloBoxF bj = {bj4.x, bj4.y, bj4.z, bj4.w};
                    hit = yolo_iou(bi, bj) > P.iou;
                }
                const unsigned long long hits = __ballot(hit);
                if (lane == 0 && hits) merged[w] |= hits;
            }
        from = i + 1;
        __syncthreads();
    }

    // ---- tail: zeros past the count, the two counts
    for (int e = kept * 6 + t; e < P.maxBoxes * 6; e += kYoloHeadThreads) out[e] = 0.0f;
    if (t == 0) {
        counts[n * 2] = static_cast<float>(kept);
        counts[n * 2 + 1] = static_cast<float>(count);
    }
}

struct YoloHeadPlan : snnhip_plan {
    snnhip_yolo_head_desc d;
    YoloHeadParams P;
    int cap = 0;

    template <typename T, int CAP>
    void launch_v(bool vec, const T* h0, const T* h1, float* rows, float* counts) {
        const dim3 grid(static_cast<unsigned>(d.N));
        if (vec) SNNHIP_LAUNCH((yolo_head_kernel<T, CAP, true>), grid, dim3(kYoloHeadThreads), 0, ctx->stream, P, h0, h1, rows, counts);
        else SNNHIP_LAUNCH((yolo_head_kernel<T, CAP, false>), grid, dim3(kYoloHeadThreads), 0, ctx->stream, P, h0, h1, rows, counts);
    }
    template <typename T>
    void launch(const snnhip_tensor* const* in, float* rows, float* counts) {
        const T* h0 = reinterpret_cast<const T*>(in[0]->data);
        const T* h1 = d.n_heads > 1 ? reinterpret_cast<const T*>(in[1]->data) : h0;
        // a 16-byte piece per candidate: its stride and every head's first byte (hence every image's) on 16 bytes
        bool vec = (static_cast<size_t>(P.vals) * sizeof(T)) % 16 == 0;
        for (int h = 0; h < d.n_heads; ++h) vec = vec && (reinterpret_cast<size_t>(in[h]->data) & 15) == 0;
        if (cap == 256) launch_v<T, 256>(vec, h0, h1, rows, counts);
        else if (cap == 1024) launch_v<T, 1024>(vec, h0, h1, rows, counts);
        else launch_v<T, 4096>(vec, h0, h1, rows, counts);
    }

    int run(const snnhip_tensor* const*, int, snnhip_tensor*) override {
        set_error("yolo_head: the plan has two outputs (the rows, the counts): run it with snnhip_plan_run_io");
        return SNNHIP_E_INVALID;
    }

    int runIO(const snnhip_tensor* const* in, int nIn, snnhip_tensor* const* out, int nOut) override {
        SNNHIP_REQUIRE(nIn == d.n_heads, "yolo_head: expects %d inputs (the heads), got %d", d.n_heads, nIn);
        SNNHIP_REQUIRE(nOut == 2, "yolo_head: expects 2 outputs (the rows, the counts), got %d", nOut);
        const int dtype = in[0]->dtype;
        SNNHIP_REQUIRE(dtype == SNNHIP_F32 || dtype == SNNHIP_F16, "yolo_head: the heads must be SNNHIP_F32 or SNNHIP_F16, got dtype %d", dtype);
        for (int h = 0; h < d.n_heads; ++h) {
            SNNHIP_REQUIRE(in[h]->dtype == dtype, "yolo_head: both heads must have one dtype, got %d and %d", dtype, in[h]->dtype);
            SNNHIP_REQUIRE(dims_match(in[h], d.N, P.grid[h], P.grid[h], P.A * P.vals), "yolo_head: head %d is %dx%dx%dx%d, the plan was built for %dx%dx%dx%d", h, in[h]->n,
                           in[h]->h, in[h]->w, in[h]->c, d.N, P.grid[h], P.grid[h], P.A * P.vals);
        }
        SNNHIP_REQUIRE(out[0]->dtype == SNNHIP_F32 && out[1]->dtype == SNNHIP_F32, "yolo_head: both outputs must be SNNHIP_F32, got %d and %d", out[0]->dtype, out[1]->dtype);
        SNNHIP_REQUIRE(dims_match(out[0], d.N, d.max_boxes, 1, 6), "yolo_head: the rows are %dx%dx%dx%d, the plan was built for %dx%dx1x6", out[0]->n, out[0]->h, out[0]->w,
                       out[0]->c, d.N, d.max_boxes);
        SNNHIP_REQUIRE(dims_match(out[1], d.N, 1, 1, 2), "yolo_head: the counts are %dx%dx%dx%d, the plan was built for %dx1x1x2", out[1]->n, out[1]->h, out[1]->w, out[1]->c, d.N);
        if (dtype == SNNHIP_F16) launch<_Float16>(in, out[0]->data, out[1]->data);
        else launch<float>(in, out[0]->data, out[1]->data);
        SNNHIP_CHECK_HIP(hipGetLastError());
        return SNNHIP_OK;
    }
};

} // namespace
} // namespace snnhip

using namespace snnhip;

extern "C" int snnhip_yolo_head_plan_create(snnhip_ctx* ctx, const snnhip_yolo_head_desc* desc, snnhip_plan** out) {
    SNNHIP_REQUIRE(ctx && desc && out, "yolo_head_plan_create: null argument");
    SNNHIP_REQUIRE(desc->N >= 1, "yolo_head desc: N = %d", desc->N);
    SNNHIP_REQUIRE(desc->n_heads == 1 || desc->n_heads == 2, "yolo_head desc: n_heads = %d (1 or 2)", desc->n_heads);
    SNNHIP_REQUIRE(desc->net_size >= 32 && desc->net_size <= 512 && desc->net_size % 32 == 0, "yolo_head desc: net_size %d (a multiple of 32, 32..512)", desc->net_size);
    SNNHIP_REQUIRE(desc->anchors_per_cell >= 1 && desc->anchors_per_cell <= kYoloHeadMaxAnchors, "yolo_head desc: anchors_per_cell = %d (1..%d)", desc->anchors_per_cell,
                   kYoloHeadMaxAnchors);
    SNNHIP_REQUIRE(desc->classes >= 1 && desc->classes <= kYoloHeadMaxClasses, "yolo_head desc: classes = %d (1..%d)", desc->classes, kYoloHeadMaxClasses);
    YoloHeadParams P = {};
    P.nHeads = desc->n_heads;
    P.A = desc->anchors_per_cell;
    P.classes = desc->classes;
    P.vals = 5 + desc->classes;
    long long M = 0;
    for (int h = 0; h < desc->n_heads; ++h) {
        const int s = desc->grid_scale[h];
        SNNHIP_REQUIRE(s >= 1 && desc->net_size % s == 0, "yolo_head desc: net_size %d is not a multiple of grid_scale[%d] = %d", desc->net_size, h, s);
        P.grid[h] = desc->net_size / s;
        P.first[h] = static_cast<int>(M);
        M += static_cast<long long>(P.grid[h]) * P.grid[h] * P.A;
        SNNHIP_REQUIRE(M <= kYoloHeadMaxCandidates, "yolo_head desc: more than %d candidates per image (net_size %d, grid_scale[%d] = %d, %d anchors per cell)",
                       kYoloHeadMaxCandidates, desc->net_size, h, s, P.A);
        P.extent[h] = static_cast<float>(s * P.grid[h]);
        for (int a = 0; a < P.A; ++a) {
            const int m = desc->masks[h * P.A + a];
            SNNHIP_REQUIRE(m >= 0 && m < 6, "yolo_head desc: masks[%d] = %d is outside the anchor table (0..5)", h * P.A + a, m);
            P.anchorW[h][a] = desc->anchors[2 * m];
            P.anchorH[h][a] = desc->anchors[2 * m + 1];
        }
    }
    for (int h = desc->n_heads; h < 3; ++h) P.first[h] = static_cast<int>(M);
    SNNHIP_REQUIRE(desc->max_boxes >= 1 && desc->max_boxes <= M, "yolo_head desc: max_boxes = %d (1..%lld, the candidates of an image)", desc->max_boxes, M);
    SNNHIP_REQUIRE(desc->conf_threshold > 0.0f && desc->conf_threshold < 1.0f && desc->iou_threshold > 0.0f && desc->iou_threshold < 1.0f,
                   "yolo_head desc: conf_threshold = %g, iou_threshold = %g (both inside (0, 1))", desc->conf_threshold, desc->iou_threshold);
    P.conf = desc->conf_threshold;
    P.iou = desc->iou_threshold;
    P.maxBoxes = desc->max_boxes;
    auto* plan = new YoloHeadPlan();
    plan->ctx = ctx;
    plan->numInputs = desc->n_heads;
    plan->numOutputs = 2;
    plan->anyDtype = true; // fp32 or fp16 heads, fp32 outputs: runIO() checks every position itself
    plan->d = *desc;
    plan->P = P;
    plan->cap = yolo_head_capacity(static_cast<int>(M));
    plan->inDims[0] = plan->outDims[0] = desc->N;
    plan->inDims[1] = plan->inDims[2] = P.grid[0];
    plan->inDims[3] = P.A * P.vals;
    plan->outDims[1] = desc->max_boxes;
    plan->outDims[2] = 1;
    plan->outDims[3] = 6;
    const double cands = static_cast<double>(desc->N) * static_cast<double>(M);
    plan->bytes = cands * P.vals * 4 + static_cast<double>(desc->N) * (desc->max_boxes * 6 + 2) * 4; // the heads once (as fp32), both outputs once
    plan->flops = cands * (8.0 + P.classes); // per candidate: the class scan, two exponentials and the confidence; the sort and the NMS depend on the data
    char buf[256];
    snprintf(buf, sizeof(buf), "yolo_head net=%d heads=%d candidates=%lld classes=%d max_boxes=%d conf=%g iou=%g cap=%d lds=%d kernel=yolo_head_kernel", desc->net_size,
             desc->n_heads, M, desc->classes, desc->max_boxes, desc->conf_threshold, desc->iou_threshold, plan->cap, yolo_head_lds_bytes(plan->cap));
    plan->desc = buf;
    *out = plan;
    return SNNHIP_OK;
}
