// capi.hip -- implementation of the C-ABI declared in include/snnhip.h: contexts, NHWC tensors, timers and the
// plan dispatcher that picks a kernel variant for each operator.
#include <cmath>
#include <new>

#include "snnhip_internal.h"

#include <atomic>
#include <chrono>
#include <cxxabi.h>
#include <map>
#include <mutex>
#include <set>
#include <string>

namespace snnhip {
std::mutex g_optMutex;
namespace {
std::map<std::string, std::string>& opt_map() {
    static std::map<std::string, std::string> m;
    return m;
}
} // namespace
const char* option(const char* name) {
    {
        std::lock_guard<std::mutex> lock(g_optMutex);
        auto it = opt_map().find(name);
        if (it != opt_map().end()) {
            // the pointer crosses the C ABI (snnhip_get_option) and outlives the lock: hand out an interned, never-freed copy so a concurrent
            // snnhip_set_option of the same name cannot leave the caller with a dangling pointer
            static std::set<std::string> interned;
            return interned.insert(it->second).first->c_str();
        }
    }
    return getenv(name);
}
} // namespace snnhip


namespace snnhip {
namespace {
bool guard_on(); // SNNHIP_GUARD=1 (below: device allocations + the guard mode)
}
static int guard_check_device(snnhip_ctx* ctx);

static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

std::vector<float> make_epilogue_table(int OC, int padTo, int useBias, const float* bias, int useBN, const float* beta, const float* gamma,
                                       const float* mean, const float* var) {
    const int n = round_up(OC, padTo);
    std::vector<float> t(static_cast<size_t>(n) * 4, 0.0f);
    for (int o = 0; o < OC; ++o) {
        t[o * 4 + 0] = (useBias && bias) ? bias[o] : 0.0f;
        if (useBN) {
            float sqrtVar = sqrtf(var[o] + 0.001f);      // vk_conv2d.comp:282
            if (sqrtVar < 0.0001f) sqrtVar = 0.0001f;     // :283
            t[o * 4 + 1] = gamma[o] / sqrtVar;
            t[o * 4 + 2] = mean[o];
            t[o * 4 + 3] = beta[o];
        } else {
            t[o * 4 + 1] = 1.0f;
        }
    }
    return t;
}

int resolve_conv_geom(const snnhip_conv2d_desc* d, bool depthwise, ConvGeom* g) {
    SNNHIP_REQUIRE(d->dtype == SNNHIP_F32 || d->dtype == SNNHIP_F16, "conv desc: dtype %d", d->dtype);
    SNNHIP_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->IC > 0 && d->OC > 0, "conv desc: non-positive dims N=%d H=%d W=%d IC=%d OC=%d", d->N, d->H,
                   d->W, d->IC, d->OC);
    SNNHIP_REQUIRE(d->kh > 0 && d->kw > 0 && d->sh > 0 && d->sw > 0, "conv desc: bad kernel/stride %dx%d / %dx%d", d->kh, d->kw, d->sh, d->sw);
    SNNHIP_REQUIRE(d->padT >= 0 && d->padB >= 0 && d->padL >= 0 && d->padR >= 0, "conv desc: negative padding");
    SNNHIP_REQUIRE(d->padMode >= 0 && d->padMode <= 3, "conv desc: padMode %d", d->padMode);
    SNNHIP_REQUIRE(d->act >= 0 && d->act <= 7, "conv desc: activation id %d", d->act);
    if (depthwise) SNNHIP_REQUIRE(d->IC == d->OC, "depthwise: IC (%d) must equal OC (%d)", d->IC, d->OC);
    g->N = d->N; g->H = d->H; g->W = d->W; g->IC = d->IC; g->OC = d->OC;
    g->kh = d->kh; g->kw = d->kw; g->sh = d->sh; g->sw = d->sw;
    const bool is1x1 = !depthwise && d->kh == 1 && d->kw == 1;
    // conv2dVulkan.cpp:154-171: the 1x1 shader gets no padding constants at all; :183-184: uPadx <- T, uPady <- L
    g->padx = is1x1 ? 0 : d->padT;
    g->pady = is1x1 ? 0 : d->padL;
    g->padMode = is1x1 ? SNNHIP_PAD_NONE : d->padMode;
    g->act = d->act;
    g->useBN = d->useBN;
    g->leaky = d->leaky;
    g->dtype = d->dtype;
    g->OH = d->OH > 0 ? d->OH : conv_out_dim(d->H, d->kh, d->sh, d->padT, d->padB);
    g->OW = d->OW > 0 ? d->OW : conv_out_dim(d->W, d->kw, d->sw, d->padT, d->padB); // reference uses offsets[0]+offsets[1] for both axes
    SNNHIP_REQUIRE(g->OH > 0 && g->OW > 0, "conv desc: empty output %dx%d", g->OH, g->OW);
    return SNNHIP_OK;
}

} // namespace snnhip

// ---- launch trace --------------------------------------------------------------------------------------------------------------------------
namespace snnhip {
namespace {
struct TraceRec {
    const void* fn;
    hipStream_t stream;
    hipEvent_t start, stop;
    int scope;
};
struct TraceScopeRec {
    std::string desc;
    double flops, bytes;
};
struct Tracer {
    std::mutex m;
    std::vector<TraceRec> recs;
    std::vector<TraceScopeRec> scopes;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    size_t used = 0;
};
Tracer& tracer() {
    static Tracer* t = new Tracer(); // leaked on purpose: events must not be destroyed after the HIP runtime has shut down
    return *t;
}
std::atomic<bool> g_traceOn{false};
thread_local int t_scope = -1;

std::string json_escape(const std::string& in) {
    std::string o;
    for (char c : in) {
        if (c == '"' || c == '\\') o += '\\';
        if (static_cast<unsigned char>(c) < 0x20) o += ' ';
        else o += c;
    }
    return o;
}
std::string demangle(const char* mangled) {
    if (!mangled) return "?";
    int st = 0;
    char* d = abi::__cxa_demangle(mangled, nullptr, nullptr, &st);
    std::string out = (st == 0 && d) ? d : mangled;
    free(d);
    return out;
}
// "void snnhip::(anonymous namespace)::conv2d_wide_kernel<4, 1, 4, 8>(Params, ...)" -> "conv2d_wide_kernel"
std::string base_name(const std::string& full) {
    if (full.compare(0, 3, "_ZN") == 0) {
        // libstdc++'s demangler does not know _Float16 (DF16_): walk the nested name ourselves -- <len><identifier>... up to the template arguments
        size_t i = 3;
        std::string last;
        while (i < full.size() && full[i] >= '0' && full[i] <= '9') {
            size_t n = 0;
            while (i < full.size() && full[i] >= '0' && full[i] <= '9') n = n * 10 + static_cast<size_t>(full[i++] - '0');
            if (i + n > full.size()) break;
            last = full.substr(i, n);
            i += n;
        }
        if (!last.empty()) return last;
    }
    size_t end = full.size();
    int depth = 0;
    // cut the parameter list: the last top-level '(' that is not "(anonymous namespace)"
    for (size_t i = 0; i < full.size(); ++i) {
        if (full[i] == '<') ++depth;
        else if (full[i] == '>') --depth;
        else if (full[i] == '(' && depth == 0 && full.compare(i, 21, "(anonymous namespace)") != 0) {
            end = i;
            break;
        }
    }
    std::string head = full.substr(0, end);
    const size_t lt = head.find('<');
    if (lt != std::string::npos) head = head.substr(0, lt);
    const size_t sp = head.rfind(' ');
    if (sp != std::string::npos) head = head.substr(sp + 1);
    const size_t cc = head.rfind("::");
    if (cc != std::string::npos) head = head.substr(cc + 2);
    return head;
}
} // namespace

bool trace_active() { return g_traceOn.load(std::memory_order_relaxed); }

int trace_events(const void* fn, hipStream_t stream, hipEvent_t* start, hipEvent_t* stop) {
    // a stream that is being captured into a graph cannot carry timing events (they would invalidate the capture and the recording run of a
    // capture_graph model would abort): such a launch goes out untimed and unrecorded -- a trace measures plans that are RUN, never the recording
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        *start = *stop = nullptr;
        return SNNHIP_OK;
    }
    Tracer& t = tracer();
    std::lock_guard<std::mutex> lock(t.m);
    if (t.used == t.pool.size()) {
        hipEvent_t a = nullptr, b = nullptr;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
            *start = *stop = nullptr; // the launch still happens, untimed
            return SNNHIP_E_HIP;
        }
        t.pool.emplace_back(a, b);
    }
    *start = t.pool[t.used].first;
    *stop = t.pool[t.used].second;
    ++t.used;
    t.recs.push_back(TraceRec{fn, stream, *start, *stop, t_scope});
    return SNNHIP_OK;
}

TraceScope::TraceScope(const std::string& desc, double flops, double bytes) {
    if (!trace_active()) return;
    Tracer& t = tracer();
    std::lock_guard<std::mutex> lock(t.m);
    t.scopes.push_back(TraceScopeRec{desc, flops, bytes});
    prev = t_scope;
    t_scope = static_cast<int>(t.scopes.size()) - 1;
}
TraceScope::TraceScope(const ::snnhip_plan* plan) : TraceScope(plan->desc, plan->flops, plan->ownBytes()) {}
TraceScope::~TraceScope() {
    if (prev != -2) t_scope = prev;
}
} // namespace snnhip

int snnhip_plan::invoke(const snnhip_tensor* const* in, int nIn, snnhip_tensor* out) {
    snnhip::TraceScope scope(this);
    return run(in, nIn, out);
}

int snnhip_plan::runIO(const snnhip_tensor* const*, int, snnhip_tensor* const*, int) {
    snnhip::set_error("plan_run_io: only a tensor_yuv plan has more than one output; this one runs through snnhip_plan_run / snnhip_plan_run_n (%s)", desc.c_str());
    return SNNHIP_E_INVALID;
}

int snnhip_plan::invokeIO(const snnhip_tensor* const* in, int nIn, snnhip_tensor* const* out, int nOut) {
    snnhip::TraceScope scope(this);
    return runIO(in, nIn, out, nOut);
}

int snnhip_plan::upload(const float* host, size_t count, float** dev) {
    void* p = nullptr;
    SNNHIP_CHECK_HIP(snnhip::dev_malloc(&p, count ? count * sizeof(float) : 4, "packed weights / table of a plan"));
    deviceAllocs.push_back(p);
    if (count) SNNHIP_CHECK_HIP(hipMemcpy(p, host, count * sizeof(float), hipMemcpyHostToDevice));
    *dev = static_cast<float*>(p);
    return SNNHIP_OK;
}

int snnhip_plan::profBegin(int step) {
    if (stepEvents.size() < static_cast<size_t>(numSteps())) {
        stepEvents.resize(numSteps());
        stepUsed.resize(numSteps(), 0);
    }
    auto& pool = stepEvents[step];
    if (stepUsed[step] == pool.size()) {
        EventPair e;
        SNNHIP_CHECK_HIP(hipEventCreate(&e.start));
        SNNHIP_CHECK_HIP(hipEventCreate(&e.stop));
        pool.push_back(e);
    }
    SNNHIP_CHECK_HIP(hipEventRecord(pool[stepUsed[step]].start, ctx->stream));
    return SNNHIP_OK;
}

int snnhip_plan::profAcquire(int step, hipEvent_t* start, hipEvent_t* stop) {
    if (stepEvents.size() < static_cast<size_t>(numSteps())) {
        stepEvents.resize(numSteps());
        stepUsed.resize(numSteps(), 0);
    }
    auto& pool = stepEvents[step];
    if (stepUsed[step] == pool.size()) {
        EventPair e;
        SNNHIP_CHECK_HIP(hipEventCreate(&e.start));
        SNNHIP_CHECK_HIP(hipEventCreate(&e.stop));
        pool.push_back(e);
    }
    *start = pool[stepUsed[step]].start;
    *stop = pool[stepUsed[step]].stop;
    ++stepUsed[step];
    return SNNHIP_OK;
}

int snnhip_plan::profEnd(int step) {
    SNNHIP_CHECK_HIP(hipEventRecord(stepEvents[step][stepUsed[step]].stop, ctx->stream));
    ++stepUsed[step];
    return SNNHIP_OK;
}

using namespace snnhip;

static std::atomic<long> g_syncSpinUs{-1}; // SNNHIP_SYNC_SPIN_US, cached: -1 = not read yet

extern "C" {

const char* snnhip_last_error(void) { return g_err; }
const char* snnhip_version(void) { return "snnhip 0.1 (gfx950)"; }

int snnhip_set_option(const char* name, const char* value) {
    SNNHIP_REQUIRE(name && strncmp(name, "SNNHIP_", 7) == 0, "set_option: option names start with SNNHIP_");
    std::lock_guard<std::mutex> lock(g_optMutex);
    if (value) opt_map()[name] = value;
    else opt_map().erase(name);
    if (strcmp(name, "SNNHIP_SYNC_SPIN_US") == 0) g_syncSpinUs.store(value ? (atol(value) > 0 ? atol(value) : 0L) : -1L); // -1: re-read the environment at the next sync
    return SNNHIP_OK;
}
const char* snnhip_get_option(const char* name) { return name ? snnhip::option(name) : nullptr; }

static int ctx_create_common(int device, hipStream_t stream, bool own, snnhip_ctx** out) {
    SNNHIP_REQUIRE(out != nullptr, "ctx_create: null out");
    int count = 0;
    SNNHIP_CHECK_HIP(hipGetDeviceCount(&count));
    SNNHIP_REQUIRE(device >= 0 && device < count, "ctx_create: device %d out of range (%d devices)", device, count);
    SNNHIP_CHECK_HIP(hipSetDevice(device));
    auto* ctx = new (std::nothrow) snnhip_ctx();
    if (!ctx) return SNNHIP_E_NOMEM;
    ctx->device = device;
    hipError_t e = hipGetDeviceProperties(&ctx->props, device);
    if (e != hipSuccess) {
        delete ctx;
        set_error("hipGetDeviceProperties failed: %s", hipGetErrorString(e));
        return SNNHIP_E_HIP;
    }
    if (own) {
        e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete ctx;
            set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
            return SNNHIP_E_HIP;
        }
        ctx->ownsStream = true;
    } else {
        ctx->stream = stream;
    }
    ctx->mainStream = ctx->stream;
    *out = ctx;
    return SNNHIP_OK;
}

int snnhip_ctx_create(int device, snnhip_ctx** out) { return ctx_create_common(device, nullptr, true, out); }

int snnhip_ctx_create_on_stream(int device, void* hip_stream, snnhip_ctx** out) {
    return ctx_create_common(device, static_cast<hipStream_t>(hip_stream), false, out);
}

int snnhip_ctx_fork(snnhip_ctx* ctx) {
    SNNHIP_REQUIRE(ctx, "ctx_fork: null ctx");
    SNNHIP_REQUIRE(ctx->stream == ctx->mainStream, "ctx_fork: already on the side stream");
    if (!ctx->sideStream) {
        SNNHIP_CHECK_HIP(hipSetDevice(ctx->device));
        SNNHIP_CHECK_HIP(hipStreamCreateWithFlags(&ctx->sideStream, hipStreamNonBlocking));
        SNNHIP_CHECK_HIP(hipEventCreateWithFlags(&ctx->forkEvent, hipEventDisableTiming));
        SNNHIP_CHECK_HIP(hipEventCreateWithFlags(&ctx->joinEvent, hipEventDisableTiming));
    }
    SNNHIP_CHECK_HIP(hipEventRecord(ctx->forkEvent, ctx->mainStream));
    SNNHIP_CHECK_HIP(hipStreamWaitEvent(ctx->sideStream, ctx->forkEvent, 0));
    ctx->stream = ctx->sideStream;
    return SNNHIP_OK;
}

int snnhip_ctx_main(snnhip_ctx* ctx) {
    SNNHIP_REQUIRE(ctx, "ctx_main: null ctx");
    ctx->stream = ctx->mainStream;
    return SNNHIP_OK;
}

int snnhip_ctx_group_begin(snnhip_ctx* ctx) {
    SNNHIP_REQUIRE(ctx, "ctx_group_begin: null context");
    return snnhip::ksplit_group_begin(ctx);
}

int snnhip_ctx_group_end(snnhip_ctx* ctx) {
    SNNHIP_REQUIRE(ctx, "ctx_group_end: null context");
    SNNHIP_CHECK_HIP(hipSetDevice(ctx->device));
    return snnhip::ksplit_group_end(ctx);
}

int snnhip_plan_groupable(const snnhip_plan* plan) { return plan && snnhip::ksplit_plan(plan) ? 1 : 0; }

int snnhip_ctx_join(snnhip_ctx* ctx) {
    SNNHIP_REQUIRE(ctx && ctx->sideStream, "ctx_join: nothing was forked");
    ctx->stream = ctx->mainStream;
    SNNHIP_CHECK_HIP(hipEventRecord(ctx->joinEvent, ctx->sideStream));
    SNNHIP_CHECK_HIP(hipStreamWaitEvent(ctx->mainStream, ctx->joinEvent, 0));
    return SNNHIP_OK;
}

int snnhip_ctx_destroy(snnhip_ctx* ctx) {
    if (!ctx) return SNNHIP_OK;
    ctx->stream = ctx->mainStream;
    if (ctx->sideStream) {
        (void) hipStreamDestroy(ctx->sideStream);
        (void) hipEventDestroy(ctx->forkEvent);
        (void) hipEventDestroy(ctx->joinEvent);
    }
    if (ctx->ownsStream && ctx->stream) (void) hipStreamDestroy(ctx->stream);
    delete ctx;
    return SNNHIP_OK;
}

int snnhip_ctx_info(snnhip_ctx* ctx, snnhip_device_info* info) {
    SNNHIP_REQUIRE(ctx && info, "ctx_info: null argument");
    memset(info, 0, sizeof(*info));
    snprintf(info->name, sizeof(info->name), "%s (%s)", ctx->props.name, ctx->props.gcnArchName);
    info->compute_units = ctx->props.multiProcessorCount;
    info->lds_bytes_per_cu = static_cast<int>(ctx->props.maxSharedMemoryPerMultiProcessor);
    info->hbm_bytes = ctx->props.totalGlobalMem;
    info->device = ctx->device;
    return SNNHIP_OK;
}

void* snnhip_ctx_stream(snnhip_ctx* ctx) { return ctx ? ctx->stream : nullptr; }

int snnhip_sync(snnhip_ctx* ctx) {
    SNNHIP_REQUIRE(ctx, "sync: null ctx");
    // An inference of the headline config is ~0.1 ms of stream time: a blocking wait (interrupt + wake-up of the host thread) can cost a tenth of
    // that.  SNNHIP_SYNC_SPIN_US > 0 polls the stream for up to that many microseconds before blocking.  Default 0 (block at once): a library must
    // not burn a host core per waiting thread unasked -- harnesses that want the polling wait opt in (bench.py times both).  The value is cached
    // (set_option / first use), not looked up per call.
    long spinUs = g_syncSpinUs.load(std::memory_order_relaxed);
    if (spinUs < 0) {
        const char* e = getenv("SNNHIP_SYNC_SPIN_US");
        spinUs = e ? atol(e) : 0L;
        if (spinUs < 0) spinUs = 0;
        g_syncSpinUs.store(spinUs, std::memory_order_relaxed);
    }
    if (spinUs > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            const hipError_t q = hipStreamQuery(ctx->mainStream);
            if (q == hipSuccess) return SNNHIP_OK;
            if (q != hipErrorNotReady) SNNHIP_CHECK_HIP(q);
            if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() >= spinUs) break;
        }
    }
    SNNHIP_CHECK_HIP(hipStreamSynchronize(ctx->mainStream)); // (side-stream work is joined into the main stream by snnhip_ctx_join)
    if (snnhip::guard_on()) return snnhip::guard_check_device(ctx); // SNNHIP_GUARD=1: every red zone of this device, SNNHIP_E_GUARD names the allocation
    return SNNHIP_OK;
}

/* ---- launch graphs ---- */

int snnhip_graph_begin_capture(snnhip_ctx* ctx) {
    SNNHIP_REQUIRE(ctx, "graph_begin_capture: null ctx");
    SNNHIP_CHECK_HIP(hipStreamBeginCapture(ctx->mainStream, hipStreamCaptureModeThreadLocal));
    return SNNHIP_OK;
}

int snnhip_graph_end_capture(snnhip_ctx* ctx, snnhip_graph** out) {
    SNNHIP_REQUIRE(ctx && out, "graph_end_capture: null argument");
    hipGraph_t graph = nullptr;
    SNNHIP_CHECK_HIP(hipStreamEndCapture(ctx->mainStream, &graph));
    SNNHIP_REQUIRE(graph != nullptr, "graph_end_capture: the capture was invalidated (a synchronising call or profiling events inside it)");
    auto* g = new snnhip_graph();
    g->ctx = ctx;
    g->graph = graph;
    size_t n = 0;
    (void) hipGraphGetNodes(graph, nullptr, &n);
    g->nodes = static_cast<int>(n);
    hipError_t e = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        set_error("hipGraphInstantiate failed: %s", hipGetErrorString(e));
        (void) hipGraphDestroy(graph);
        delete g;
        return SNNHIP_E_HIP;
    }
    *out = g;
    return SNNHIP_OK;
}

int snnhip_graph_launch(snnhip_graph* g) {
    SNNHIP_REQUIRE(g && g->exec, "graph_launch: null graph");
    SNNHIP_CHECK_HIP(hipGraphLaunch(g->exec, g->ctx->mainStream));
    return SNNHIP_OK;
}

int snnhip_graph_num_nodes(const snnhip_graph* g) { return g ? g->nodes : 0; }

int snnhip_graph_destroy(snnhip_graph* g) {
    if (!g) return SNNHIP_OK;
    if (g->exec) (void) hipGraphExecDestroy(g->exec);
    if (g->graph) (void) hipGraphDestroy(g->graph);
    delete g;
    return SNNHIP_OK;
}

/* ---- device allocations + the guard mode (SNNHIP_GUARD=1) ---- */

extern "C++" {
namespace snnhip {
namespace {
constexpr size_t kGuardZone = 64 * 1024; // bytes of 0xFF in front of and behind every allocation (a multiple of 256: the user pointer keeps hipMalloc's alignment)
struct GuardRec {
    char* base;       // what hipMalloc returned: [front zone][user bytes][slack to 16 + back zone]
    size_t bytes;     // user bytes
    size_t backBytes; // bytes of the zone behind the user region (kGuardZone + the slack that rounds the region up to 16)
    int device;
    std::string what;
};
struct GuardZoneDesc {
    const unsigned char* p;
    unsigned long long bytes;
};
std::mutex g_guardMutex;
std::map<void*, GuardRec>& guard_map() {
    static std::map<void*, GuardRec> m;
    return m;
}
std::atomic<int> g_guardOn{-1};

bool guard_on() {
    int v = g_guardOn.load(std::memory_order_relaxed);
    if (v < 0) {
        const char* e = getenv("SNNHIP_GUARD"); // (the environment only, read once at the first allocation: a process is guarded or it is not)
        v = (e && atoi(e) != 0) ? 1 : 0;
        g_guardOn.store(v, std::memory_order_relaxed);
    }
    return v == 1;
}

// one block per red zone: the lowest offset whose byte is not 0xFF, as (zone index << 40 | offset), minimum over everything
__global__ void guard_check_kernel(const GuardZoneDesc* zones, unsigned long long* first) {
    const GuardZoneDesc z = zones[blockIdx.x];
    for (unsigned long long i = threadIdx.x; i < z.bytes; i += blockDim.x)
        if (z.p[i] != 0xFFu) {
            atomicMin(first, (static_cast<unsigned long long>(blockIdx.x) << 40) | i);
            break;
        }
}
__global__ void guard_poke_kernel(unsigned char* p) { *p = 0x5A; }
} // namespace

hipError_t dev_malloc_bytes(void** p, size_t bytes, const char* what) {
    if (!guard_on()) return hipMalloc(p, (bytes + 15) & ~static_cast<size_t>(15));
    const size_t user = (bytes + 15) & ~static_cast<size_t>(15);
    void* base = nullptr;
    const hipError_t e = hipMalloc(&base, kGuardZone + user + kGuardZone);
    if (e != hipSuccess) return e;
    // zones AND contents are filled with 0xFF: nothing reads as a plausible number before it is written.  The fill runs on a helper stream of its own and is
    // waited for here (a kernel launched right behind the allocation on a context's non-blocking stream raced a null-stream fill: the guard leg's first
    // finding was its own).  Not the null stream: a legacy-stream memset + synchronise is illegal while another stream of the thread records a hipGraph;
    // if the runtime refuses the helper stream's wait for that reason the allocation fails with a message that says so (allocate before the capture).
    hipError_t m = hipSuccess;
    {
        static std::mutex fillMutex;
        static std::map<int, hipStream_t> fillStreams;
        int dev = 0;
        (void) hipGetDevice(&dev);
        std::lock_guard<std::mutex> lock(fillMutex);
        hipStream_t& fs = fillStreams[dev];
        if (!fs) m = hipStreamCreateWithFlags(&fs, hipStreamNonBlocking);
        if (m == hipSuccess) m = hipMemsetAsync(base, 0xFF, kGuardZone + user + kGuardZone, fs);
        if (m == hipSuccess) m = hipStreamSynchronize(fs);
    }
    if (m != hipSuccess) {
        (void) hipFree(base);
        set_error("SNNHIP_GUARD: the poison fill of a new allocation (%s, %zu bytes) failed: %s%s", what ? what : "", bytes, hipGetErrorString(m),
                  (m == hipErrorStreamCaptureUnsupported || m == hipErrorStreamCaptureImplicit) ? " -- guarded allocations cannot be made while a stream capture is in progress" : "");
        return m;
    }
    GuardRec r;
    r.base = static_cast<char*>(base);
    r.bytes = bytes;
    r.backBytes = (user - bytes) + kGuardZone;
    r.what = what ? what : "";
    r.device = 0;
    (void) hipGetDevice(&r.device);
    *p = r.base + kGuardZone;
    std::lock_guard<std::mutex> lock(g_guardMutex);
    guard_map()[*p] = r;
    return hipSuccess;
}

hipError_t dev_free(void* p) {
    if (!p) return hipSuccess;
    if (guard_on()) {
        std::lock_guard<std::mutex> lock(g_guardMutex);
        auto it = guard_map().find(p);
        if (it != guard_map().end()) {
            void* base = it->second.base;
            guard_map().erase(it);
            return hipFree(base);
        }
    }
    return hipFree(p);
}

// every red zone of the allocations on ctx's device; SNNHIP_E_GUARD + a message naming the first damaged allocation (its zone is re-poisoned so that the
// next check reports new damage only).  The stream is drained first: called from snnhip_sync, never inside a capture.
static int guard_check_device(snnhip_ctx* ctx) {
    std::vector<GuardZoneDesc> zones;
    std::vector<void*> owner;
    // The registry stays locked for the WHOLE check: a dev_free of a same-device allocation from another thread (a pool replica, a plan being destroyed)
    // would otherwise let the check kernel read freed memory.  dev_free / dev_malloc_bytes wait; nothing in here calls them.
    std::lock_guard<std::mutex> lock(g_guardMutex);
    struct DeviceRestore { // the caller's current device is put back on every path out
        int prev = -1;
        DeviceRestore() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
        ~DeviceRestore() { if (prev >= 0) (void) hipSetDevice(prev); }
    } restoreDevice;
    {
        for (const auto& kv : guard_map()) {
            const GuardRec& r = kv.second;
            if (r.device != ctx->device) continue;
            zones.push_back({reinterpret_cast<const unsigned char*>(r.base), static_cast<unsigned long long>(kGuardZone)});
            owner.push_back(kv.first);
            zones.push_back({reinterpret_cast<const unsigned char*>(r.base) + kGuardZone + r.bytes, static_cast<unsigned long long>(r.backBytes)});
            owner.push_back(kv.first);
        }
    }
    if (zones.empty()) return SNNHIP_OK;
    SNNHIP_CHECK_HIP(hipSetDevice(ctx->device));
    void* dz = nullptr;
    SNNHIP_CHECK_HIP(hipMalloc(&dz, zones.size() * sizeof(GuardZoneDesc) + 8));
    unsigned long long* dfirst = reinterpret_cast<unsigned long long*>(static_cast<char*>(dz) + zones.size() * sizeof(GuardZoneDesc));
    unsigned long long first = ~0ull;
    hipError_t e = hipMemcpy(dz, zones.data(), zones.size() * sizeof(GuardZoneDesc), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dfirst, &first, 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(guard_check_kernel, dim3(static_cast<unsigned>(zones.size())), dim3(256), 0, ctx->mainStream, static_cast<const GuardZoneDesc*>(dz), dfirst);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->mainStream);
    if (e == hipSuccess) e = hipMemcpy(&first, dfirst, 8, hipMemcpyDeviceToHost);
    (void) hipFree(dz);
    SNNHIP_CHECK_HIP(e);
    if (first == ~0ull) return SNNHIP_OK;
    const size_t zi = static_cast<size_t>(first >> 40), off = static_cast<size_t>(first & ((1ull << 40) - 1));
    std::string what;
    size_t bytes = 0;
    {
        auto it = guard_map().find(owner[zi]);
        if (it != guard_map().end()) {
            what = it->second.what;
            bytes = it->second.bytes;
        }
    }
    if (hipMemsetAsync(const_cast<unsigned char*>(zones[zi].p), 0xFF, zones[zi].bytes, ctx->mainStream) == hipSuccess) (void) hipStreamSynchronize(ctx->mainStream);
    if (zi & 1)
        set_error("SNNHIP_GUARD: a kernel wrote %zu byte(s) past the END of a device allocation (%s, %zu bytes, device %d)", off + 1, what.c_str(), bytes, ctx->device);
    else
        set_error("SNNHIP_GUARD: a kernel wrote %zu byte(s) in FRONT of a device allocation (%s, %zu bytes, device %d)", kGuardZone - off, what.c_str(), bytes, ctx->device);
    return SNNHIP_E_GUARD;
}
} // namespace snnhip
} // extern "C++"

int snnhip_guard_active(void) { return snnhip::guard_on() ? 1 : 0; }

int snnhip_guard_check(snnhip_ctx* ctx) {
    SNNHIP_REQUIRE(ctx, "guard_check: null ctx");
    if (!snnhip::guard_on()) return SNNHIP_OK;
    SNNHIP_CHECK_HIP(hipStreamSynchronize(ctx->mainStream));
    return snnhip::guard_check_device(ctx);
}

int snnhip_guard_selftest(snnhip_ctx* ctx, snnhip_tensor* t, long offset) {
    SNNHIP_REQUIRE(ctx && t && t->data, "guard_selftest: null argument");
    SNNHIP_REQUIRE(snnhip::guard_on() && t->owns, "guard_selftest: needs SNNHIP_GUARD=1 and a tensor of snnhip_tensor_alloc");
    SNNHIP_REQUIRE(offset >= -static_cast<long>(snnhip::kGuardZone) && offset < static_cast<long>(snnhip::kGuardZone) && offset != -0x7fffffffL,
                   "guard_selftest: offset %ld outside the red zones", offset);
    unsigned char* p = reinterpret_cast<unsigned char*>(t->data) + (offset >= 0 ? static_cast<long>(t->bytes()) + offset : offset);
    hipLaunchKernelGGL(snnhip::guard_poke_kernel, dim3(1), dim3(1), 0, ctx->stream, p);
    SNNHIP_CHECK_HIP(hipGetLastError());
    return SNNHIP_OK;
}

/* ---- tensors ---- */

int snnhip_tensor_alloc(snnhip_ctx* ctx, int n, int h, int w, int c, int dtype, snnhip_tensor** out) {
    SNNHIP_REQUIRE(ctx && out, "tensor_alloc: null argument");
    SNNHIP_REQUIRE(dtype == SNNHIP_F32 || dtype == SNNHIP_F16 || dtype == SNNHIP_U8 || dtype == SNNHIP_U16, "tensor_alloc: dtype %d not implemented", dtype);
    SNNHIP_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0, "tensor_alloc: bad dims %dx%dx%dx%d", n, h, w, c);
    auto* t = new (std::nothrow) snnhip_tensor();
    if (!t) return SNNHIP_E_NOMEM;
    t->ctx = ctx; t->n = n; t->h = h; t->w = w; t->c = c; t->owns = true; t->dtype = dtype;
    void* p = nullptr;
    const size_t nbytes = t->bytes(); // (rounded up to whole 16-byte vectors by the allocator; under SNNHIP_GUARD the red zone starts right behind the last element)
    char what[96];
    snprintf(what, sizeof(what), "tensor %dx%dx%dx%d dtype %d", n, h, w, c, dtype);
    hipError_t e = snnhip::dev_malloc(&p, nbytes, what);
    if (e != hipSuccess) {
        delete t;
        set_error("hipMalloc(%zu) failed: %s", nbytes, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? SNNHIP_E_NOMEM : SNNHIP_E_HIP;
    }
    t->data = static_cast<float*>(p);
    *out = t;
    return SNNHIP_OK;
}

int snnhip_tensor_wrap(snnhip_ctx* ctx, void* device_ptr, int n, int h, int w, int c, int dtype, snnhip_tensor** out) {
    SNNHIP_REQUIRE(ctx && out && device_ptr, "tensor_wrap: null argument");
    SNNHIP_REQUIRE(dtype == SNNHIP_F32 || dtype == SNNHIP_F16 || dtype == SNNHIP_U8 || dtype == SNNHIP_U16, "tensor_wrap: dtype %d not implemented", dtype);
    SNNHIP_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0, "tensor_wrap: bad dims %dx%dx%dx%d", n, h, w, c);
    SNNHIP_REQUIRE((reinterpret_cast<uintptr_t>(device_ptr) & 15) == 0, "tensor_wrap: pointer must be 16-byte aligned");
    auto* t = new (std::nothrow) snnhip_tensor();
    if (!t) return SNNHIP_E_NOMEM;
    t->ctx = ctx; t->n = n; t->h = h; t->w = w; t->c = c; t->owns = false; t->dtype = dtype;
    t->data = static_cast<float*>(device_ptr);
    *out = t;
    return SNNHIP_OK;
}

int snnhip_tensor_free(snnhip_tensor* t) {
    if (!t) return SNNHIP_OK;
    if (t->owns && t->data) (void) snnhip::dev_free(t->data);
    delete t;
    return SNNHIP_OK;
}

int snnhip_tensor_dims(const snnhip_tensor* t, int dims[4]) {
    SNNHIP_REQUIRE(t && dims, "tensor_dims: null argument");
    dims[0] = t->n; dims[1] = t->h; dims[2] = t->w; dims[3] = t->c;
    return SNNHIP_OK;
}

void* snnhip_tensor_data(const snnhip_tensor* t) { return t ? t->data : nullptr; }
size_t snnhip_tensor_bytes(const snnhip_tensor* t) { return t ? t->bytes() : 0; }
int snnhip_tensor_dtype(const snnhip_tensor* t) { return t ? t->dtype : -1; }

// fp32 <-> fp16 on the host (API edge only): round to nearest even, like the GPU's image stores
int snnhip_tensor_upload(snnhip_tensor* t, const float* host) {
    SNNHIP_REQUIRE(t && host, "tensor_upload: null argument");
    SNNHIP_REQUIRE(t->dtype != SNNHIP_U8, "tensor_upload: 8-bit image tensors take snnhip_tensor_upload_raw");
    SNNHIP_REQUIRE(t->dtype != SNNHIP_U16, "tensor_upload: 16-bit frame tensors take snnhip_tensor_upload_raw");
    if (t->dtype == SNNHIP_F16) {
        std::vector<_Float16> tmp(t->count());
        for (size_t i = 0; i < tmp.size(); ++i) tmp[i] = static_cast<_Float16>(host[i]);
        SNNHIP_CHECK_HIP(hipMemcpyAsync(t->data, tmp.data(), t->bytes(), hipMemcpyHostToDevice, t->ctx->stream));
        SNNHIP_CHECK_HIP(hipStreamSynchronize(t->ctx->stream));
        return SNNHIP_OK;
    }
    SNNHIP_CHECK_HIP(hipMemcpyAsync(t->data, host, t->bytes(), hipMemcpyHostToDevice, t->ctx->stream));
    SNNHIP_CHECK_HIP(hipStreamSynchronize(t->ctx->stream));
    return SNNHIP_OK;
}

int snnhip_tensor_download(const snnhip_tensor* t, float* host) {
    SNNHIP_REQUIRE(t && host, "tensor_download: null argument");
    SNNHIP_REQUIRE(t->dtype != SNNHIP_U8, "tensor_download: not available for 8-bit image tensors");
    SNNHIP_REQUIRE(t->dtype != SNNHIP_U16, "tensor_download: not available for 16-bit frame tensors (snnhip_tensor_download_raw)");
    if (t->dtype == SNNHIP_F16) {
        std::vector<_Float16> tmp(t->count());
        SNNHIP_CHECK_HIP(hipMemcpyAsync(tmp.data(), t->data, t->bytes(), hipMemcpyDeviceToHost, t->ctx->stream));
        SNNHIP_CHECK_HIP(hipStreamSynchronize(t->ctx->stream));
        for (size_t i = 0; i < tmp.size(); ++i) host[i] = static_cast<float>(tmp[i]);
        return (snnhip::guard_on() && t->ctx->stream == t->ctx->mainStream) ? snnhip::guard_check_device(t->ctx) : SNNHIP_OK;
    }
    SNNHIP_CHECK_HIP(hipMemcpyAsync(host, t->data, t->bytes(), hipMemcpyDeviceToHost, t->ctx->stream));
    SNNHIP_CHECK_HIP(hipStreamSynchronize(t->ctx->stream));
    return (snnhip::guard_on() && t->ctx->stream == t->ctx->mainStream) ? snnhip::guard_check_device(t->ctx) : SNNHIP_OK; // (a download ends most tests: SNNHIP_GUARD checks here too)
}

int snnhip_tensor_upload_raw(snnhip_tensor* t, const void* host, size_t nbytes) {
    SNNHIP_REQUIRE(t && host, "tensor_upload_raw: null argument");
    SNNHIP_REQUIRE(nbytes == t->bytes(), "tensor_upload_raw: %zu bytes given, the tensor holds %zu", nbytes, t->bytes());
    SNNHIP_CHECK_HIP(hipMemcpyAsync(t->data, host, nbytes, hipMemcpyHostToDevice, t->ctx->stream));
    SNNHIP_CHECK_HIP(hipStreamSynchronize(t->ctx->stream));
    return SNNHIP_OK;
}

int snnhip_tensor_download_raw(const snnhip_tensor* t, void* host, size_t nbytes) {
    SNNHIP_REQUIRE(t && host, "tensor_download_raw: null argument");
    SNNHIP_REQUIRE(nbytes == t->bytes(), "tensor_download_raw: %zu bytes asked for, the tensor holds %zu", nbytes, t->bytes());
    SNNHIP_CHECK_HIP(hipMemcpyAsync(host, t->data, nbytes, hipMemcpyDeviceToHost, t->ctx->stream));
    SNNHIP_CHECK_HIP(hipStreamSynchronize(t->ctx->stream));
    return (snnhip::guard_on() && t->ctx->stream == t->ctx->mainStream) ? snnhip::guard_check_device(t->ctx) : SNNHIP_OK;
}

// C4HW4 <-> NHWC conversion happens on the host: it is an API-edge format (uploads of test inputs, dumps), never
// on the inference path.
int snnhip_tensor_upload_c4hw4(snnhip_tensor* t, const float* c4) {
    SNNHIP_REQUIRE(t && c4, "tensor_upload_c4hw4: null argument");
    std::vector<float> nhwc(t->count());
    const size_t hw = static_cast<size_t>(t->h) * t->w;
    const int planes = up_div(t->c, 4);
    for (int n = 0; n < t->n; ++n) {
        const float* src = c4 + static_cast<size_t>(n) * planes * hw * 4;
        float* dst = nhwc.data() + static_cast<size_t>(n) * hw * t->c;
        for (size_t i = 0; i < hw; ++i)
            for (int c = 0; c < t->c; ++c) dst[i * t->c + c] = src[(static_cast<size_t>(c / 4) * hw + i) * 4 + (c % 4)];
    }
    return snnhip_tensor_upload(t, nhwc.data());
}

int snnhip_tensor_download_c4hw4(const snnhip_tensor* t, float* c4) {
    SNNHIP_REQUIRE(t && c4, "tensor_download_c4hw4: null argument");
    std::vector<float> nhwc(t->count());
    int rc = snnhip_tensor_download(t, nhwc.data());
    if (rc != SNNHIP_OK) return rc;
    const size_t hw = static_cast<size_t>(t->h) * t->w;
    const int planes = up_div(t->c, 4);
    memset(c4, 0, static_cast<size_t>(t->n) * planes * hw * 4 * sizeof(float));
    for (int n = 0; n < t->n; ++n) {
        float* dst = c4 + static_cast<size_t>(n) * planes * hw * 4;
        const float* src = nhwc.data() + static_cast<size_t>(n) * hw * t->c;
        for (size_t i = 0; i < hw; ++i)
            for (int c = 0; c < t->c; ++c) dst[(static_cast<size_t>(c / 4) * hw + i) * 4 + (c % 4)] = src[i * t->c + c];
    }
    return SNNHIP_OK;
}

__global__ void fill_kernel(float* p, size_t n, float v) {
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * blockDim.x) p[i] = v;
}

__global__ void fill_half_kernel(_Float16* p, size_t n, float v) {
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * blockDim.x) p[i] = static_cast<_Float16>(v);
}

int snnhip_tensor_fill(snnhip_tensor* t, float value) {
    SNNHIP_REQUIRE(t, "tensor_fill: null argument");
    SNNHIP_REQUIRE(t->dtype != SNNHIP_U8, "tensor_fill: not available for 8-bit image tensors");
    SNNHIP_REQUIRE(t->dtype != SNNHIP_U16, "tensor_fill: not available for 16-bit frame tensors");
    size_t n = t->count();
    unsigned blocks = static_cast<unsigned>(std::min<size_t>((n + 255) / 256, 4096));
    if (t->dtype == SNNHIP_F16)
        SNNHIP_LAUNCH(fill_half_kernel, dim3(blocks), dim3(256), 0, t->ctx->stream, reinterpret_cast<_Float16*>(t->data), n, value);
    else
        SNNHIP_LAUNCH(fill_kernel, dim3(blocks), dim3(256), 0, t->ctx->stream, t->data, n, value);
    SNNHIP_CHECK_HIP(hipGetLastError());
    return SNNHIP_OK;
}

/* ---- plans ---- */

static int check_conv_args(snnhip_ctx* ctx, const snnhip_conv2d_desc* desc, const float* w, const float* bn_beta, const float* bn_gamma,
                           const float* bn_mean, const float* bn_var, snnhip_plan** out) {
    SNNHIP_REQUIRE(ctx && desc && w && out, "plan_create: null argument");
    if (desc->useBN) SNNHIP_REQUIRE(bn_beta && bn_gamma && bn_mean && bn_var, "plan_create: useBN set but a BN array is null");
    return SNNHIP_OK;
}

int snnhip_conv2d_plan_create(snnhip_ctx* ctx, const snnhip_conv2d_desc* desc, const float* w_oihw, const float* bias, const float* bn_beta,
                              const float* bn_gamma, const float* bn_mean, const float* bn_var, snnhip_plan** out) {
    int rc = check_conv_args(ctx, desc, w_oihw, bn_beta, bn_gamma, bn_mean, bn_var, out);
    if (rc != SNNHIP_OK) return rc;
    ConvGeom g;
    rc = resolve_conv_geom(desc, false, &g);
    if (rc != SNNHIP_OK) return rc;
    SNNHIP_CHECK_HIP(hipSetDevice(ctx->device));
    std::vector<float> epi = make_epilogue_table(g.OC, 16, desc->useBias, bias, desc->useBN, bn_beta, bn_gamma, bn_mean, bn_var);
    // image-producing layers (OC <= 4) go to the 4x4x1-MFMA kernel, GEMM-shaped layers to the fp32-MFMA implicit GEMM; everything else
    // (and anything they decline) to the direct VALU kernel.
    rc = make_conv2d_rowfold_plan(ctx, g, w_oihw, epi, out); // fp16, wide kernel, k * OC <= 32: kernel columns folded into the MFMA's N
    if (rc == SNNHIP_E_UNSUPPORTED) rc = make_conv2d_thin_plan(ctx, g, w_oihw, epi, out);
    if (rc == SNNHIP_E_UNSUPPORTED) rc = make_conv2d_mfma_plan(ctx, g, w_oihw, epi, out);
    if (rc == SNNHIP_E_UNSUPPORTED && g.dtype != SNNHIP_F32) {
        // A half-precision layer whose OWN input or output tensor has 2^31 or more elements (Candy's 64 -> 32 up-convolution at 32 images: the x2-upsampled,
        // padded 64-channel tensor it nominally reads has 2.3e9 -- a tensor that never exists, graph rule D evaluates the layer on the low-resolution one):
        // the layer gets a description-only plan the chain planner can fuse from (geometry, weights, epilogue table); running it alone fails with a message.
        const double inCount = static_cast<double>(g.N) * g.H * g.W * g.IC, outCount = static_cast<double>(g.N) * g.OH * g.OW * g.OC;
        if (inCount >= 2147483647.0 || outCount >= 2147483647.0) {
            struct OversizeConvPlan : ConvPlanBase {
                int run(const snnhip_tensor* const*, int, snnhip_tensor*) override {
                    set_error("conv2d: %s -- a tensor of 2^31 or more elements: this layer only runs fused behind its UpSampling2D / Pad (graph rule D)", desc.c_str());
                    return SNNHIP_E_UNSUPPORTED;
                }
            };
            auto* plan = new OversizeConvPlan();
            plan->ctx = ctx;
            plan->g = g;
            plan->w_oihw.assign(w_oihw, w_oihw + static_cast<size_t>(g.OC) * g.IC * g.kh * g.kw);
            plan->epi4 = epi;
            plan->dtype = g.dtype;
            plan->inDims[0] = g.N; plan->inDims[1] = g.H; plan->inDims[2] = g.W; plan->inDims[3] = g.IC;
            plan->outDims[0] = g.N; plan->outDims[1] = g.OH; plan->outDims[2] = g.OW; plan->outDims[3] = g.OC;
            plan->flops = 2.0 * g.kh * g.kw * g.IC * g.OC * static_cast<double>(g.OH) * g.OW * g.N;
            plan->bytes = 2.0 * (inCount + outCount + static_cast<double>(g.OC) * g.IC * g.kh * g.kw);
            char buf[200];
            snprintf(buf, sizeof(buf), "conv2d_mfma_f16 k=%dx%d s=%d ic=%d oc=%d OVERSIZE (%.3g input elements): description only, runs fused (rule D)", g.kh, g.kw, g.sh, g.IC, g.OC, inCount);
            plan->desc = buf;
            *out = plan;
            return SNNHIP_OK;
        }
        set_error("conv2d: no fp16 kernel takes this shape (k=%dx%d stride %d, %d->%d)", g.kh, g.kw, g.sh, g.IC, g.OC);
        return rc;
    }
    if (rc == SNNHIP_E_UNSUPPORTED) rc = make_conv2d_generic_plan(ctx, g, w_oihw, epi, out);
    return rc;
}

int snnhip_depthwise_plan_create(snnhip_ctx* ctx, const snnhip_conv2d_desc* desc, const float* w_chw, const float* bias, const float* bn_beta,
                                 const float* bn_gamma, const float* bn_mean, const float* bn_var, snnhip_plan** out) {
    int rc = check_conv_args(ctx, desc, w_chw, bn_beta, bn_gamma, bn_mean, bn_var, out);
    if (rc != SNNHIP_OK) return rc;
    ConvGeom g;
    rc = resolve_conv_geom(desc, true, &g);
    if (rc != SNNHIP_OK) return rc;
    SNNHIP_CHECK_HIP(hipSetDevice(ctx->device));
    // the depthwise shader always reads the bias buffer (vk_depthwise.comp:79); a null pointer means zeros
    std::vector<float> epi = make_epilogue_table(g.OC, 16, bias != nullptr, bias, desc->useBN, bn_beta, bn_gamma, bn_mean, bn_var);
    return make_depthwise_plan(ctx, g, w_chw, epi, out);
}

int snnhip_dense_plan_create(snnhip_ctx* ctx, const snnhip_dense_desc* desc, const float* w_flat, const float* bias, snnhip_plan** out) {
    SNNHIP_REQUIRE(ctx && desc && w_flat && out, "dense_plan_create: null argument");
    SNNHIP_REQUIRE(desc->batch > 0 && desc->in_units > 0 && desc->out_units > 0, "dense desc: bad dims batch=%d in=%d out=%d", desc->batch,
                   desc->in_units, desc->out_units);
    SNNHIP_REQUIRE(desc->act >= 0 && desc->act <= 6, "dense desc: activation id %d", desc->act);
    SNNHIP_CHECK_HIP(hipSetDevice(ctx->device));
    return make_dense_plan(ctx, *desc, w_flat, bias, out);
}

int snnhip_subpixel_plan_create(snnhip_ctx* ctx, const snnhip_subpixel_desc* desc, snnhip_plan** out) {
    SNNHIP_REQUIRE(ctx && desc && out, "subpixel_plan_create: null argument");
    SNNHIP_REQUIRE(desc->N > 0 && desc->H > 0 && desc->W > 0 && desc->C > 0 && desc->factor > 0, "subpixel desc: bad dims");
    SNNHIP_REQUIRE(desc->mode == SNNHIP_SUBPIXEL_D2S || desc->mode == SNNHIP_SUBPIXEL_VK_QUIRK, "subpixel desc: mode %d", desc->mode);
    return make_subpixel_plan(ctx, *desc, out);
}

int snnhip_chain_plan_create(snnhip_ctx* ctx, snnhip_plan* const* plans, int n, snnhip_plan** out) {
    SNNHIP_REQUIRE(ctx && plans && out && n > 0, "chain_plan_create: bad argument");
    for (int i = 0; i < n; ++i) SNNHIP_REQUIRE(plans[i] != nullptr, "chain_plan_create: plan %d is null", i);
    SNNHIP_CHECK_HIP(hipSetDevice(ctx->device));
    return make_chain_plan(ctx, plans, n, out);
}

int snnhip_plan_run_n(snnhip_plan* plan, const snnhip_tensor* const* inputs, int n_in, snnhip_tensor* out) {
    SNNHIP_REQUIRE(plan && inputs && out && n_in > 0, "plan_run: null argument");
    for (int i = 0; i < n_in; ++i) SNNHIP_REQUIRE(inputs[i] && inputs[i]->data, "plan_run: input %d is null", i);
    SNNHIP_REQUIRE(out->data, "plan_run: output has no storage");
    if (plan->numOutputs != 1) return plan->run(inputs, n_in, out); // a tensor_yuv plan: its run() refuses and names snnhip_plan_run_io
    // a raw frame tensor (SNNHIP_U8 / SNNHIP_U16) is accepted exactly where the plan declares one
    for (int i = 0; i < n_in; ++i) {
        SNNHIP_REQUIRE(inputs[i]->dtype != SNNHIP_U8 || plan->rawInput == SNNHIP_U8, "plan_run: input %d is an 8-bit image tensor (%s)", i, plan->desc.c_str());
        SNNHIP_REQUIRE(inputs[i]->dtype != SNNHIP_U16 || plan->rawInput == SNNHIP_U16, "plan_run: input %d is a 16-bit frame tensor (%s)", i, plan->desc.c_str());
    }
    if (plan->rawOutput == SNNHIP_U8) SNNHIP_REQUIRE(out->dtype == SNNHIP_U8, "plan_run: the output must be an 8-bit tensor (%s), got dtype %d", plan->desc.c_str(), out->dtype);
    else SNNHIP_REQUIRE(out->dtype != SNNHIP_U8, "plan_run: the output is an 8-bit image tensor (%s)", plan->desc.c_str());
    if (plan->rawOutput == SNNHIP_U16) SNNHIP_REQUIRE(out->dtype == SNNHIP_U16, "plan_run: the output must be a 16-bit tensor (%s), got dtype %d", plan->desc.c_str(), out->dtype);
    else SNNHIP_REQUIRE(out->dtype != SNNHIP_U16, "plan_run: the output is a 16-bit frame tensor (%s)", plan->desc.c_str());
    if (!plan->anyDtype) {
        const int outDtype = plan->rawOutput >= 0 ? plan->rawOutput : plan->dtype;
        for (int i = 0; i < n_in; ++i) {
            const int inDtype = plan->rawInput >= 0 && i == 0 ? plan->rawInput : plan->dtype;
            SNNHIP_REQUIRE(inputs[i]->dtype == inDtype, "plan_run: input %d has dtype %d, the plan (%s) was built for %d", i, inputs[i]->dtype, plan->desc.c_str(), inDtype);
        }
        SNNHIP_REQUIRE(out->dtype == outDtype, "plan_run: output has dtype %d, the plan (%s) was built for %d", out->dtype, plan->desc.c_str(), outDtype);
    }
    if (plan->profiling && !plan->profilesItself()) {
        int rc = plan->profBegin(0);
        if (rc != SNNHIP_OK) return rc;
        rc = plan->invoke(inputs, n_in, out);
        if (rc != SNNHIP_OK) return rc;
        return plan->profEnd(0);
    }
    return plan->invoke(inputs, n_in, out);
}

int snnhip_plan_run_io(snnhip_plan* plan, const snnhip_tensor* const* inputs, int n_in, snnhip_tensor* const* outputs, int n_out) {
    SNNHIP_REQUIRE(plan && inputs && outputs && n_in > 0 && n_out > 0, "plan_run_io: null argument");
    SNNHIP_REQUIRE(plan->numOutputs > 1, "plan_run_io: only a tensor_yuv plan has more than one output; this one runs through snnhip_plan_run / snnhip_plan_run_n (%s)",
                   plan->desc.c_str());
    for (int i = 0; i < n_in; ++i) SNNHIP_REQUIRE(inputs[i] && inputs[i]->data, "plan_run_io: input %d is null", i);
    for (int i = 0; i < n_out; ++i) SNNHIP_REQUIRE(outputs[i] && outputs[i]->data, "plan_run_io: output %d is null or has no storage", i);
    if (plan->profiling && !plan->profilesItself()) {
        int rc = plan->profBegin(0);
        if (rc != SNNHIP_OK) return rc;
        rc = plan->invokeIO(inputs, n_in, outputs, n_out);
        if (rc != SNNHIP_OK) return rc;
        return plan->profEnd(0);
    }
    return plan->invokeIO(inputs, n_in, outputs, n_out);
}

int snnhip_plan_num_steps(const snnhip_plan* plan) { return plan ? plan->numSteps() : 0; }

int snnhip_plan_step_describe(const snnhip_plan* plan, int step, char* buf, size_t buflen) {
    SNNHIP_REQUIRE(plan && buf && buflen > 0 && step >= 0 && step < plan->numSteps(), "plan_step_describe: bad argument");
    snprintf(buf, buflen, "%s", plan->stepDesc(step).c_str());
    return SNNHIP_OK;
}

int snnhip_plan_step_cost(const snnhip_plan* plan, int step, double* flops, double* bytes) {
    SNNHIP_REQUIRE(plan && step >= 0 && step < plan->numSteps(), "plan_step_cost: bad argument");
    double f = 0, b = 0;
    plan->stepCost(step, &f, &b);
    if (flops) *flops = f;
    if (bytes) *bytes = b;
    return SNNHIP_OK;
}

int snnhip_plan_profile_enable(snnhip_plan* plan, int enable) {
    SNNHIP_REQUIRE(plan, "plan_profile_enable: null plan");
    plan->profiling = enable != 0;
    return SNNHIP_OK;
}

int snnhip_plan_profile_read(snnhip_plan* plan, int step, double* total_ms, int* launches) {
    SNNHIP_REQUIRE(plan && total_ms && launches && step >= 0 && step < plan->numSteps(), "plan_profile_read: bad argument");
    *total_ms = 0;
    *launches = 0;
    if (plan->stepEvents.size() <= static_cast<size_t>(step)) return SNNHIP_OK;
    for (size_t i = 0; i < plan->stepUsed[step]; ++i) {
        auto& e = plan->stepEvents[step][i];
        SNNHIP_CHECK_HIP(hipEventSynchronize(e.stop));
        float ms = 0;
        SNNHIP_CHECK_HIP(hipEventElapsedTime(&ms, e.start, e.stop));
        *total_ms += ms;
        ++*launches;
    }
    plan->stepUsed[step] = 0;
    return SNNHIP_OK;
}

int snnhip_plan_run(snnhip_plan* plan, const snnhip_tensor* in, snnhip_tensor* out) { return snnhip_plan_run_n(plan, &in, 1, out); }

int snnhip_plan_output_dims(const snnhip_plan* plan, int dims[4]) {
    SNNHIP_REQUIRE(plan && dims, "plan_output_dims: null argument");
    memcpy(dims, plan->outDims, sizeof(int) * 4);
    return SNNHIP_OK;
}

int snnhip_plan_describe(const snnhip_plan* plan, char* buf, size_t buflen) {
    SNNHIP_REQUIRE(plan && buf && buflen > 0, "plan_describe: null argument");
    snprintf(buf, buflen, "%s", plan->desc.c_str());
    return SNNHIP_OK;
}

int snnhip_plan_cost(const snnhip_plan* plan, double* flops, double* bytes) {
    SNNHIP_REQUIRE(plan, "plan_cost: null argument");
    if (flops) *flops = plan->flops;
    if (bytes) *bytes = plan->bytes;
    return SNNHIP_OK;
}

int snnhip_plan_destroy(snnhip_plan* plan) {
    delete plan;
    return SNNHIP_OK;
}

/* ---- launch trace ---- */

int snnhip_trace_begin(void) {
    Tracer& t = tracer();
    std::lock_guard<std::mutex> lock(t.m);
    t.recs.clear();
    t.scopes.clear();
    t.used = 0;
    g_traceOn.store(true);
    return SNNHIP_OK;
}

int snnhip_trace_end(void) {
    g_traceOn.store(false);
    return SNNHIP_OK;
}

int snnhip_trace_report(char* buf, size_t buflen, size_t* needed) {
    SNNHIP_REQUIRE(!g_traceOn.load(), "trace_report: call snnhip_trace_end first");
    Tracer& t = tracer();
    std::lock_guard<std::mutex> lock(t.m);
    struct Inst {
        std::string name;
        long launches = 0;
        double ms = 0, flops = 0, bytes = 0;
        double mfmaFlops = 0; // what the matrix pipe executes where that differs from the algorithmic count ("mfma_flops=" in the plan's description: Winograd, pre-summed taps)
        long mainLaunches = 0;
        std::vector<std::string> plans;
    };
    std::map<const void*, Inst> insts;
    std::vector<float> dur(t.recs.size(), 0.0f);
    for (size_t i = 0; i < t.recs.size(); ++i) {
        const TraceRec& r = t.recs[i];
        if (!r.start) continue;
        SNNHIP_CHECK_HIP(hipEventSynchronize(r.stop));
        SNNHIP_CHECK_HIP(hipEventElapsedTime(&dur[i], r.start, r.stop));
        Inst& in = insts[r.fn];
        if (in.name.empty()) in.name = demangle(hipKernelNameRefByPtr(r.fn, r.stream));
        ++in.launches;
        in.ms += dur[i];
    }
    // a scope's algorithmic cost is booked on its longest launch (a convolution next to its split-K reduce pass, a dense layer next to its softmax)
    std::vector<int> mainOf(t.scopes.size(), -1);
    for (size_t i = 0; i < t.recs.size(); ++i) {
        const int sc = t.recs[i].scope;
        if (sc < 0 || !t.recs[i].start) continue;
        if (mainOf[sc] < 0 || dur[i] > dur[mainOf[sc]]) mainOf[sc] = static_cast<int>(i);
    }
    for (size_t sc = 0; sc < t.scopes.size(); ++sc) {
        if (mainOf[sc] < 0) continue;
        Inst& in = insts[t.recs[mainOf[sc]].fn];
        in.flops += t.scopes[sc].flops;
        in.bytes += t.scopes[sc].bytes;
        {
            const size_t at = t.scopes[sc].desc.find("mfma_flops=");
            if (at != std::string::npos) in.mfmaFlops += strtod(t.scopes[sc].desc.c_str() + at + 11, nullptr);
        }
        ++in.mainLaunches;
        bool seen = false;
        for (const auto& d : in.plans) seen = seen || d == t.scopes[sc].desc;
        if (!seen && in.plans.size() < 64) in.plans.push_back(t.scopes[sc].desc);
    }
    std::map<std::string, std::vector<const Inst*>> byBase;
    for (const auto& kv : insts) byBase[base_name(kv.second.name)].push_back(&kv.second);
    std::string js = "{\"launches\": " + std::to_string(t.recs.size()) + ", \"kernels\": [";
    bool firstK = true;
    char num[256];
    for (const auto& kv : byBase) {
        long launches = 0, mainLaunches = 0;
        double ms = 0, flops = 0, bytes = 0, mfmaFlops = 0;
        for (const Inst* in : kv.second) {
            launches += in->launches;
            mainLaunches += in->mainLaunches;
            ms += in->ms;
            flops += in->flops;
            bytes += in->bytes;
            mfmaFlops += in->mfmaFlops;
        }
        snprintf(num, sizeof(num), "\"launches\": %ld, \"main_launches\": %ld, \"total_ms\": %.9g, \"flops\": %.9g, \"bytes\": %.9g, \"mfma_flops\": %.9g", launches, mainLaunches, ms,
                 flops, bytes, mfmaFlops);
        js += std::string(firstK ? "" : ", ") + "{\"function\": \"" + json_escape(kv.first) + "\", " + num + ", \"instances\": [";
        firstK = false;
        bool firstI = true;
        for (const Inst* in : kv.second) {
            snprintf(num, sizeof(num), "\"launches\": %ld, \"main_launches\": %ld, \"total_ms\": %.9g, \"flops\": %.9g, \"bytes\": %.9g, \"mfma_flops\": %.9g", in->launches,
                     in->mainLaunches, in->ms, in->flops, in->bytes, in->mfmaFlops);
            js += std::string(firstI ? "" : ", ") + "{\"name\": \"" + json_escape(in->name) + "\", " + num + ", \"plans\": [";
            firstI = false;
            for (size_t k = 0; k < in->plans.size(); ++k) js += std::string(k ? ", " : "") + "\"" + json_escape(in->plans[k]) + "\"";
            js += "]}";
        }
        js += "]}";
    }
    js += "]}";
    if (needed) *needed = js.size() + 1;
    if (buf && buflen > 0) {
        const size_t n = js.size() < buflen - 1 ? js.size() : buflen - 1;
        memcpy(buf, js.data(), n);
        buf[n] = 0;
    }
    return SNNHIP_OK;
}

/* ---- timers ---- */

int snnhip_timer_create(snnhip_ctx* ctx, snnhip_timer** out) {
    SNNHIP_REQUIRE(ctx && out, "timer_create: null argument");
    auto* t = new (std::nothrow) snnhip_timer();
    if (!t) return SNNHIP_E_NOMEM;
    t->ctx = ctx;
    hipError_t e = hipEventCreate(&t->start);
    if (e == hipSuccess) e = hipEventCreate(&t->stop);
    if (e != hipSuccess) {
        if (t->start) (void) hipEventDestroy(t->start);
        delete t;
        set_error("hipEventCreate failed: %s", hipGetErrorString(e));
        return SNNHIP_E_HIP;
    }
    *out = t;
    return SNNHIP_OK;
}

int snnhip_timer_start(snnhip_timer* t) {
    SNNHIP_REQUIRE(t, "timer_start: null");
    SNNHIP_CHECK_HIP(hipEventRecord(t->start, t->ctx->stream));
    return SNNHIP_OK;
}

int snnhip_timer_stop(snnhip_timer* t) {
    SNNHIP_REQUIRE(t, "timer_stop: null");
    SNNHIP_CHECK_HIP(hipEventRecord(t->stop, t->ctx->stream));
    return SNNHIP_OK;
}

int snnhip_timer_elapsed_ms(snnhip_timer* t, float* ms) {
    SNNHIP_REQUIRE(t && ms, "timer_elapsed: null");
    SNNHIP_CHECK_HIP(hipEventSynchronize(t->stop));
    SNNHIP_CHECK_HIP(hipEventElapsedTime(ms, t->start, t->stop));
    return SNNHIP_OK;
}

int snnhip_timer_destroy(snnhip_timer* t) {
    if (!t) return SNNHIP_OK;
    (void) hipEventDestroy(t->start);
    (void) hipEventDestroy(t->stop);
    delete t;
    return SNNHIP_OK;
}

} // extern "C"
