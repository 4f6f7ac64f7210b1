// ecamd_runtime.hip -- what every other file of libecamd.so stands on, and the thin C ABI over the HIP
// runtime: the thread's error text (dev_fail, ecamd_last_error), ecamd_tune, device count / get / set,
// ecamd_malloc ... ecamd_event_*, ecamd_scatter_fragments and ecamd_fill_splitmix; the per-(device,
// stream) contexts (side stream, scratch slots), StagedUpload, and the "upload a table once" helper
// (upload_table, OnceTable).  Contracts in ecamd_internal.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../host/tune.hpp"
#include "ecamd.h"
#include "ecamd_internal.hpp"
#include "ecamd_kernels.hpp"

using namespace ecamd;

namespace {

thread_local std::string g_err;

// Per-(device, caller stream) context of the framed calls: the side stream (knob frame_tail_fork)
// with its fork / join events, and the CRC scratch slots of ecamd_frame_api.hip.  side_fork makes
// the side stream wait for everything issued so far to the caller's stream; side_join makes the
// caller's stream wait for everything issued to the side stream since.  The payload tails of a
// padded framed encode, and the LDS-table rest of a copy-through map, run there beside the launch
// over the whole tiles; the two write disjoint bytes.
//
// Callers that create and destroy streams (a proxy's per-request streams) must not grow this map
// for the life of the process: ecamd_stream_destroy releases the stream's context, and past
// kStreamCtxMax contexts every new one first releases the IDLE contexts of other streams -- no
// framed call or fork in progress (busy), and every event recorded for them complete (done: the
// end of the last framed call, join: the side stream's last work), so neither the side stream nor
// a scratch slot can still be in use.  Only our own events are queried, never a caller's stream
// (which may have been destroyed behind our back).
struct StreamCtx {
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr, done = nullptr;
    int busy = 0;  // framed calls (StreamUse) and forks not yet joined
    uint32_t* scratch[kStreamScratchSlots] = {};
    size_t scratch_words[kStreamScratchSlots] = {};
};
constexpr size_t kStreamCtxMax = 16;
std::mutex g_ctx_mu;
auto& g_ctx = *new std::map<std::pair<int, void*>, StreamCtx>();  // never destroyed: no HIP call at exit

bool ctx_idle(const StreamCtx& c)
{
    if (c.busy) return false;
    for (hipEvent_t e : {c.join, c.done})
        if (e && hipEventQuery(e) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
    return true;
}

// Releases an idle context's resources (the caller holds g_ctx_mu and erases the entry).
void ctx_release(int dev, StreamCtx& c)
{
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (cur != dev) (void)hipSetDevice(dev);
    if (c.side) (void)hipStreamDestroy(c.side);
    for (hipEvent_t e : {c.fork, c.join, c.done})
        if (e) (void)hipEventDestroy(e);
    for (uint32_t* p : c.scratch)
        if (p) (void)hipFree(p);
    if (cur >= 0 && cur != dev) (void)hipSetDevice(cur);
    (void)hipGetLastError();
    c = StreamCtx{};
}

// The context of (dev, stream), created on first use; g_ctx_mu held.
StreamCtx& ctx_of(int dev, void* stream)
{
    const auto key = std::make_pair(dev, stream);
    auto it = g_ctx.find(key);
    if (it != g_ctx.end()) return it->second;
    if (g_ctx.size() >= kStreamCtxMax)
        for (auto jt = g_ctx.begin(); jt != g_ctx.end();) {
            if (ctx_idle(jt->second)) {
                ctx_release(jt->first.first, jt->second);
                jt = g_ctx.erase(jt);
            } else {
                ++jt;
            }
        }
    return g_ctx[key];
}

}  // namespace

namespace ecamd {

int dev_fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int upload_table(const char* what, const void* host, size_t bytes, const void** dev)
{
    void* d = nullptr;
    hipError_t err = hipMalloc(&d, bytes);
    if (err == hipSuccess && (err = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice)) != hipSuccess) (void)hipFree(d);
    if (err != hipSuccess) return dev_fail(ECAMD_EHIP, "%s: %s", what, hipGetErrorString(err));
    *dev = d;
    return 0;
}

OnceTable::~OnceTable()
{
    if (dev) (void)hipFree(const_cast<uint32_t*>(dev));
}

int stream_use_begin(int dev, void* stream)
{
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    ctx_of(dev, stream).busy++;
    return 0;
}

void stream_use_end(int dev, void* stream)
{
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    const auto it = g_ctx.find(std::make_pair(dev, stream));
    if (it == g_ctx.end()) return;
    StreamCtx& c = it->second;
    // everything this call enqueued on the caller's stream (scratch reads included) is behind `done`
    if (!c.done && hipEventCreateWithFlags(&c.done, hipEventDisableTiming) != hipSuccess) c.done = nullptr;
    if (c.done) (void)hipEventRecord(c.done, static_cast<hipStream_t>(stream));
    (void)hipGetLastError();
    if (c.busy > 0) c.busy--;
}

int stream_scratch(int dev, void* stream, int slot, size_t words, uint32_t** out)
{
    if (slot < 0 || slot >= kStreamScratchSlots) return dev_fail(ECAMD_EINVAL, "scratch slot %d", slot);
    const size_t want = std::max<size_t>(words, 1);
    // Growing a slot drains this stream and frees the old buffer: done with g_ctx_mu RELEASED, so framed
    // calls on other streams never wait behind this one (the slot is taken out of the context first;
    // the caller is inside a StreamUse, so the context itself is not released meanwhile)
    uint32_t* old = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_ctx_mu);
        StreamCtx& c = ctx_of(dev, stream);
        if (c.scratch_words[slot] >= words && c.scratch[slot]) {
            *out = c.scratch[slot];
            return 0;
        }
        old = c.scratch[slot];
        c.scratch[slot] = nullptr;
        c.scratch_words[slot] = 0;
    }
    if (old) {  // calls on one stream are ordered: the old slot is free once the stream drains
        HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
        HIP_TRY(hipFree(old));
    }
    uint32_t* p = nullptr;
    HIP_TRY(hipMalloc(&p, want * sizeof(uint32_t)));
    // zeroed once: the small-launch CRC's counter must start at 0 (it resets itself after every launch)
    HIP_TRY(hipMemsetAsync(p, 0, want * sizeof(uint32_t), static_cast<hipStream_t>(stream)));
    uint32_t* spare = nullptr;  // another thread on the same stream installed one meanwhile
    {
        std::lock_guard<std::mutex> lk(g_ctx_mu);
        StreamCtx& c = ctx_of(dev, stream);
        if (c.scratch[slot] && c.scratch_words[slot] >= want) {
            spare = p;
            p = c.scratch[slot];
        } else {
            spare = c.scratch[slot];
            c.scratch[slot] = p;
            c.scratch_words[slot] = want;
        }
    }
    if (spare) {
        HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
        HIP_TRY(hipFree(spare));
    }
    *out = p;
    return 0;
}

int side_fork(int dev, void* stream, void** side)
{
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    StreamCtx& e = ctx_of(dev, stream);
    if (!e.side) {  // all three or none: a half-made context would record on null events later
        hipStream_t s = nullptr;
        hipEvent_t f = nullptr, j = nullptr;
        hipError_t rc = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (rc == hipSuccess) rc = hipEventCreateWithFlags(&f, hipEventDisableTiming);
        if (rc == hipSuccess) rc = hipEventCreateWithFlags(&j, hipEventDisableTiming);
        if (rc != hipSuccess) {
            if (s) (void)hipStreamDestroy(s);
            if (f) (void)hipEventDestroy(f);
            (void)hipGetLastError();
            return dev_fail(ECAMD_EHIP, "side stream: %s", hipGetErrorString(rc));
        }
        e.side = s;
        e.fork = f;
        e.join = j;
    }
    HIP_TRY(hipEventRecord(e.fork, static_cast<hipStream_t>(stream)));
    HIP_TRY(hipStreamWaitEvent(e.side, e.fork, 0));
    e.busy++;
    *side = e.side;
    return 0;
}

int side_join(int dev, void* stream)
{
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    const auto it = g_ctx.find(std::make_pair(dev, stream));
    if (it == g_ctx.end() || !it->second.side) return dev_fail(ECAMD_EHIP, "side_join without side_fork");
    StreamCtx& e = it->second;
    if (e.busy > 0) e.busy--;
    HIP_TRY(hipEventRecord(e.join, e.side));
    HIP_TRY(hipStreamWaitEvent(static_cast<hipStream_t>(stream), e.join, 0));
    return 0;
}

// ecamd_stream_destroy: the stream's contexts go with it (after its work, which may read them).
void stream_forget(void* stream)
{
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    for (auto it = g_ctx.begin(); it != g_ctx.end();) {
        if (it->first.second == stream && !it->second.busy) {
            (void)hipStreamSynchronize(static_cast<hipStream_t>(stream));
            if (it->second.side) (void)hipStreamSynchronize(it->second.side);
            ctx_release(it->first.first, it->second);
            it = g_ctx.erase(it);
        } else {
            ++it;
        }
    }
    (void)hipGetLastError();
}

int stream_contexts()
{
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    return static_cast<int>(g_ctx.size());
}

// StagedUpload: a small host table (stripe list / pointer table) goes up asynchronously on the
// caller's stream, ahead of the launches that read it, from one of kStagedSlots (pinned host,
// device) buffer pairs per (device, stream); a slot is reused only after the event recorded behind
// its launches (end()) has fired, so back-to-back calls do not drain the stream.  Locking is per
// ring and only around claiming / releasing a slot: the event wait, the upload and the launches
// run unlocked, so batches on other streams or devices never wait behind this one.
struct StagedSlot {
    void* host = nullptr;
    void* dev = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;
    bool busy = false;  // claimed by a StagedUpload between begin() and end()
};
constexpr int kStagedSlots = 4;
struct StagedRing {
    std::mutex mu;
    std::condition_variable freed;
    StagedSlot slot[kStagedSlots];
    int next = 0;
};
namespace {
std::mutex g_staged_mu;
std::map<std::pair<int, void*>, std::unique_ptr<StagedRing>> g_staged;  // (device, stream)
}  // namespace

int StagedUpload::begin(int device, void* stream, const void* src, size_t bytes)
{
    end(stream_);  // a second begin() releases the first slot
    {
        std::lock_guard<std::mutex> lk(g_staged_mu);
        auto& r = g_staged[{device, stream}];
        if (!r) r.reset(new StagedRing());
        ring_ = r.get();
    }
    {
        std::unique_lock<std::mutex> lk(ring_->mu);
        StagedSlot* sc = &ring_->slot[ring_->next];
        ring_->next = (ring_->next + 1) % kStagedSlots;
        ring_->freed.wait(lk, [sc] { return !sc->busy; });
        sc->busy = true;
        slot_ = sc;
        stream_ = stream;
    }
    StagedSlot& sc = *slot_;
    if (sc.done) HIP_TRY(hipEventSynchronize(sc.done));
    else HIP_TRY(hipEventCreateWithFlags(&sc.done, hipEventDisableTiming));
    const size_t need = std::max<size_t>(bytes, 16);
    if (sc.cap < need) {
        if (sc.host) HIP_TRY(hipHostFree(sc.host));
        if (sc.dev) HIP_TRY(hipFree(sc.dev));
        sc.host = sc.dev = nullptr;
        sc.cap = 0;
        HIP_TRY(hipHostMalloc(&sc.host, need, hipHostMallocDefault));
        HIP_TRY(hipMalloc(&sc.dev, need));
        sc.cap = need;
    }
    std::memcpy(sc.host, src, bytes);
    HIP_TRY(hipMemcpyAsync(sc.dev, sc.host, bytes, hipMemcpyHostToDevice, static_cast<hipStream_t>(stream)));
    dev = sc.dev;
    return 0;
}

int StagedUpload::end(void* stream)
{
    if (!slot_) return 0;
    hipError_t e = hipSuccess;
    if (slot_->done) e = hipEventRecord(slot_->done, static_cast<hipStream_t>(stream));
    {
        std::lock_guard<std::mutex> lk(ring_->mu);
        slot_->busy = false;
    }
    ring_->freed.notify_all();
    slot_ = nullptr;
    ring_ = nullptr;
    dev = nullptr;
    if (e != hipSuccess) return dev_fail(ECAMD_EHIP, "hipEventRecord: %s", hipGetErrorString(e));
    return 0;
}

}  // namespace ecamd

extern "C" {

int ecamd_tune(const char* key, int value)
{
    if (!key) return dev_fail(ECAMD_EINVAL, "null key");
    const TuneSet r = tune_set(g_tune, key, value);  // the knobs and their rules: host/tune_knobs.def
    if (!r.knob) return dev_fail(ECAMD_EINVAL, "unknown tuning key %s", key);
    if (!r.stored) return dev_fail(ECAMD_EINVAL, "%s must be %s", key, r.knob->must);
    return 0;
}

int ecamd_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int ecamd_get_device(int* dev)
{
    if (!dev) return dev_fail(ECAMD_EINVAL, "null device pointer");
    HIP_TRY(hipGetDevice(dev));
    return 0;
}

int ecamd_set_device(int dev)
{
    HIP_TRY(hipSetDevice(dev));
    return 0;
}

const char* ecamd_last_error(void) { return g_err.c_str(); }

int ecamd_scatter_fragments(const void* d_src, int64_t stripe_stride, int64_t frag_stride,
                            int64_t frag_len, int nfrags, int nstripes, const int* dst_dev,
                            void* const* d_dst, const int64_t* dst_stride, void* stream)
{
    int dev = 0;
    int rc = dev_ensure(&dev);
    if (rc) return rc;
    if (!d_src || !dst_dev || !d_dst || !dst_stride || nfrags < 0 || nstripes < 0 || frag_len < 0)
        return dev_fail(ECAMD_EINVAL, "bad scatter arguments");
    if (nfrags == 0 || nstripes == 0 || frag_len == 0) return 0;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    // Check every destination before anything is queued: a bad request copies nothing.
    for (int f = 0; f < nfrags; f++) {
        const int to = dst_dev[f];
        if (to < 0 || to >= ndev) return dev_fail(ECAMD_EINVAL, "fragment %d: bad device %d", f, to);
        if (!d_dst[f] || dst_stride[f] < frag_len)
            return dev_fail(ECAMD_EINVAL, "fragment %d: bad destination / stride", f);
    }
    // Peer links (from, to) opened once per process; copy lanes are per (from, to) streams created
    // on the source device, so copies to different peers run at once, one xGMI link each, instead
    // of one after another on the caller's stream.
    static std::mutex mu;
    static std::vector<std::pair<int, int>> enabled;
    static std::map<std::pair<int, int>, hipStream_t> lanes;
    const int mode = g_tune.scatter_lanes;
    std::vector<int> order;  // destination devices in first-use order
    for (int f = 0; f < nfrags; f++)
        if (std::find(order.begin(), order.end(), dst_dev[f]) == order.end()) order.push_back(dst_dev[f]);
    std::vector<std::pair<int, hipStream_t>> used;  // (destination, lane) of this call
    {
        std::lock_guard<std::mutex> lk(mu);
        for (const int to : order) {
            if (to != dev && std::find(enabled.begin(), enabled.end(), std::make_pair(dev, to)) == enabled.end()) {
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, dev, to) != hipSuccess || !can) {
                    int f = 0;
                    while (dst_dev[f] != to) f++;
                    return dev_fail(ECAMD_EINVAL, "fragment %d: no peer path from device %d to %d", f, dev, to);
                }
                hipError_t e = hipDeviceEnablePeerAccess(to, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
                    int f = 0;
                    while (dst_dev[f] != to) f++;
                    return dev_fail(ECAMD_EHIP, "fragment %d: hipDeviceEnablePeerAccess(%d -> %d): %s", f, dev,
                                to, hipGetErrorString(e));
                }
                (void)hipGetLastError();
                enabled.emplace_back(dev, to);
            }
            const bool lane = mode == 1 || (mode == 0 && to != dev);
            if (!lane) continue;
            hipStream_t& s = lanes[std::make_pair(dev, to)];
            if (!s) HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
            used.emplace_back(to, s);
        }
    }
    const hipStream_t caller = static_cast<hipStream_t>(stream);
    // fork: every lane starts after the work already queued on the caller's stream
    hipEvent_t fork = nullptr;
    if (!used.empty()) {
        HIP_TRY(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
        const hipError_t e = hipEventRecord(fork, caller);
        if (e != hipSuccess) {
            (void)hipEventDestroy(fork);
            return dev_fail(ECAMD_EHIP, "scatter fork: %s", hipGetErrorString(e));
        }
    }
    std::vector<hipEvent_t> joins;
    auto lane_of = [&](int to) -> hipStream_t {
        for (const auto& u : used)
            if (u.first == to) return u.second;
        return caller;
    };
    for (const int to : order) {
        const hipStream_t s = lane_of(to);
        if (s != caller) {
            const hipError_t e = hipStreamWaitEvent(s, fork, 0);
            if (e != hipSuccess) {
                rc = dev_fail(ECAMD_EHIP, "device %d lane: hipStreamWaitEvent: %s", to, hipGetErrorString(e));
                break;
            }
        }
        for (int f = 0; f < nfrags && rc == 0; f++) {
            if (dst_dev[f] != to) continue;
            // One strided copy per fragment: nstripes rows of frag_len bytes (xGMI DMA when to != dev).
            const hipError_t e = hipMemcpy2DAsync(
                d_dst[f], static_cast<size_t>(dst_stride[f]),
                static_cast<const uint8_t*>(d_src) + f * frag_stride, static_cast<size_t>(stripe_stride),
                static_cast<size_t>(frag_len), static_cast<size_t>(nstripes), hipMemcpyDefault, s);
            if (e != hipSuccess)
                rc = dev_fail(ECAMD_EHIP, "fragment %d -> device %d: hipMemcpy2DAsync: %s", f, to,
                          hipGetErrorString(e));
        }
        if (s != caller) {  // join: the caller's stream continues once this lane's copies landed
            hipEvent_t j = nullptr;
            hipError_t e = hipEventCreateWithFlags(&j, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventRecord(j, s);
            if (e == hipSuccess) e = hipStreamWaitEvent(caller, j, 0);
            if (j) joins.push_back(j);
            if (e != hipSuccess && rc == 0)
                rc = dev_fail(ECAMD_EHIP, "device %d lane: join: %s", to, hipGetErrorString(e));
        }
        if (rc) break;
    }
    // events may be destroyed while pending: their resources go once they complete
    for (hipEvent_t j : joins) (void)hipEventDestroy(j);
    if (fork) (void)hipEventDestroy(fork);
    return rc;
}

int ecamd_fill_splitmix(void* base, int64_t stripe_stride, int64_t frag_stride, int nfrags,
                        int64_t blocksize, int nstripes, int stripe0, uint64_t seed_base,
                        void* stream)
{
    int dev = 0;
    int rc = dev_ensure(&dev);
    if (rc) return rc;
    if (!aligned16(base) || stripe_stride % 8 || frag_stride % 8)
        return dev_fail(ECAMD_EINVAL, "fill: base must be 16-byte and strides 8-byte aligned");
    FillArgs f{static_cast<uint8_t*>(base), stripe_stride, frag_stride, blocksize, nfrags,
               nstripes, stripe0, seed_base};
    int64_t total = ((blocksize + 7) / 8) * nfrags * static_cast<int64_t>(nstripes);
    int64_t grid = std::min<int64_t>((total + 255) / 256, static_cast<int64_t>(dev_cu_count(dev)) * 16);
    hipLaunchKernelGGL(splitmix_fill_kernel, dim3(static_cast<int>(std::max<int64_t>(grid, 1))),
                       dim3(256), 0, static_cast<hipStream_t>(stream), f);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ecamd_malloc(void** d_ptr, int64_t bytes)
{
    int rc = dev_ensure(nullptr);
    if (rc) return rc;
    HIP_TRY(hipMalloc(d_ptr, static_cast<size_t>(bytes)));
    return 0;
}

int ecamd_malloc_host_writable(void** d_ptr, int64_t bytes)
{
    int rc = dev_ensure(nullptr);
    if (rc) return rc;
    if (!d_ptr || bytes <= 0) return dev_fail(ECAMD_EINVAL, "bad host-writable allocation");
    void* p = nullptr;
    // uncached on the GPU side: the kernel always sees what the host wrote last, no stale cache lines
    HIP_TRY(hipExtMallocWithFlags(&p, static_cast<size_t>(bytes), hipDeviceMallocUncached));
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) != hipSuccess || attr.hostPointer != p) {
        (void)hipGetLastError();
        (void)hipFree(p);
        return dev_fail(ECAMD_EINVAL, "device memory is not host-accessible here (no large BAR)");
    }
    *d_ptr = p;
    return 0;
}

int ecamd_free(void* d_ptr)
{
    HIP_TRY(hipFree(d_ptr));
    return 0;
}

int ecamd_memcpy_h2d(void* d_dst, const void* h_src, int64_t bytes)
{
    HIP_TRY(hipMemcpy(d_dst, h_src, static_cast<size_t>(bytes), hipMemcpyHostToDevice));
    return 0;
}

int ecamd_memcpy_d2h(void* h_dst, const void* d_src, int64_t bytes)
{
    HIP_TRY(hipMemcpy(h_dst, d_src, static_cast<size_t>(bytes), hipMemcpyDeviceToHost));
    return 0;
}

int ecamd_memset(void* d_ptr, int value, int64_t bytes)
{
    // Complete on return (hipMemset alone may still be running when the host moves on, and
    // streams made by ecamd_stream_create do not order against the null stream).
    HIP_TRY(hipMemset(d_ptr, value, static_cast<size_t>(bytes)));
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}

int ecamd_memcpy_async(void* dst, const void* src, int64_t bytes, int kind, void* stream)
{
    hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice
                      : kind == 1 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    HIP_TRY(hipMemcpyAsync(dst, src, static_cast<size_t>(bytes), k, static_cast<hipStream_t>(stream)));
    return 0;
}

int ecamd_host_alloc(void** h_ptr, int64_t bytes)
{
    int rc = dev_ensure(nullptr);
    if (rc) return rc;
    HIP_TRY(hipHostMalloc(h_ptr, static_cast<size_t>(bytes), hipHostMallocDefault));
    return 0;
}

int ecamd_host_free(void* h_ptr)
{
    HIP_TRY(hipHostFree(h_ptr));
    return 0;
}

int ecamd_synchronize(void)
{
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}

int ecamd_stream_create(void** stream)
{
    int rc = dev_ensure(nullptr);
    if (rc) return rc;
    hipStream_t s;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = s;
    return 0;
}

int ecamd_stream_destroy(void* stream)
{
    ecamd::stream_forget(stream);
    HIP_TRY(hipStreamDestroy(static_cast<hipStream_t>(stream)));
    return 0;
}

int ecamd_stream_destroy_unmanaged(void* stream)
{
    HIP_TRY(hipStreamDestroy(static_cast<hipStream_t>(stream)));
    return 0;
}

int ecamd_stream_synchronize(void* stream)
{
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return 0;
}

int ecamd_stream_query(void* stream)
{
    const hipError_t e = hipStreamQuery(static_cast<hipStream_t>(stream));
    if (e == hipSuccess) return 0;
    if (e == hipErrorNotReady) return 1;
    return ECAMD_EHIP;
}

int ecamd_stream_contexts(void) { return ecamd::stream_contexts(); }

int ecamd_event_create(void** ev)
{
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    *ev = e;
    return 0;
}

int ecamd_event_destroy(void* ev)
{
    HIP_TRY(hipEventDestroy(static_cast<hipEvent_t>(ev)));
    return 0;
}

int ecamd_event_record(void* ev, void* stream)
{
    HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(ev), static_cast<hipStream_t>(stream)));
    return 0;
}

int ecamd_event_elapsed_ms(void* start, void* stop, float* ms)
{
    HIP_TRY(hipEventSynchronize(static_cast<hipEvent_t>(stop)));
    HIP_TRY(hipEventElapsedTime(ms, static_cast<hipEvent_t>(start), static_cast<hipEvent_t>(stop)));
    return 0;
}

}  // extern "C"
