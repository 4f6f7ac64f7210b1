// ecamd_device.hip -- host side of libecamd.so: device discovery, fragment-map planning
// (row groups / column chunks sized to the 160 KiB LDS of a gfx950 CU), launch geometry and
// the cached liberasurecode_rs_vand encode/decode/reconstruct maps.  C ABI in include/ecamd.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <numeric>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../host/bitslice.hpp"
#include "../host/crc.hpp"
#include "../host/gf16.hpp"
#include "../host/tables.hpp"
#include "../host/tune.hpp"
#include "ecamd.h"
#include "ecamd_host.h"
#include "ecamd_internal.hpp"
#include "ecamd_kernels.hpp"
#include "ecamd_server_slots.hpp"
#include "ecamd_frame.hpp"

using namespace ecamd;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(ECAMD_EHIP, "%s: %s", #expr, hipGetErrorString(e_));               \
    } while (0)

struct DeviceInfo {
    int cus = 0;
    bool lds_attr_set = false;
};

std::mutex g_dev_mu;
int g_ndev = -1;
std::vector<DeviceInfo> g_dev;

int ensure_device(int* dev_out)
{
    std::lock_guard<std::mutex> lk(g_dev_mu);
    if (g_ndev < 0) {
        tune_from_env();
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
        g_ndev = n;
        g_dev.assign(std::max(n, 0), DeviceInfo());
    }
    if (g_ndev <= 0)
        return fail(ECAMD_ENODEV, "liberasurecode_amd: no HIP device (MI355X) available; "
                                  "this backend has no CPU fallback");
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    DeviceInfo& di = g_dev[dev];
    if (di.cus == 0) {
        HIP_TRY(hipDeviceGetAttribute(&di.cus, hipDeviceAttributeMultiprocessorCount, dev));
        if (di.cus <= 0) di.cus = 256;
    }
    if (!di.lds_attr_set) {
        // Allow the full 160 KiB of gfx950 LDS as dynamic shared memory.
#define K_(W, P, N) reinterpret_cast<const void*>(&gf16_apply_kernel<W, P, N, false>)
        const void* ks[] = {K_(2, false, false), K_(4, false, false), K_(8, false, false),
                            K_(2, true, false),  K_(4, true, false),  K_(8, true, false),
                            K_(2, false, true),  K_(4, false, true),  K_(8, false, true),
                            K_(2, true, true),   K_(4, true, true),   K_(8, true, true),
                            reinterpret_cast<const void*>(&gf16_copy_apply_kernel<2>),
                            reinterpret_cast<const void*>(&gf16_copy_apply_kernel<4>),
                            reinterpret_cast<const void*>(&gf16_copy_apply_kernel<8>)};
#undef K_
        for (const void* k : ks)
            HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
#define K_(W, KG, CH, PF, N) reinterpret_cast<const void*>(&gf16_stream_kernel<W, KG, CH, PF, N>)
#define KG_(W, CH, PF, N) K_(W, 1, CH, PF, N), K_(W, 2, CH, PF, N), K_(W, 3, CH, PF, N), \
                          K_(W, 4, CH, PF, N), K_(W, 5, CH, PF, N)
        const void* sk[] = {KG_(2, 1, true, false),  KG_(4, 1, true, false),  KG_(8, 1, true, false),
                            KG_(2, 1, false, false), KG_(4, 1, false, false), KG_(8, 1, false, false),
                            KG_(2, 2, true, false),  KG_(4, 2, true, false),  KG_(2, 2, false, false),
                            KG_(4, 2, false, false), KG_(2, 1, false, true),  KG_(4, 1, false, true),
                            KG_(8, 1, false, true)};
#undef KG_
#undef K_
#define KP_(W) reinterpret_cast<const void*>(&gf16_ptrs_stream_kernel<W, 1>),                 \
               reinterpret_cast<const void*>(&gf16_ptrs_stream_kernel<W, 2>),                 \
               reinterpret_cast<const void*>(&gf16_ptrs_stream_kernel<W, 3>),                 \
               reinterpret_cast<const void*>(&gf16_ptrs_stream_kernel<W, 4>),                 \
               reinterpret_cast<const void*>(&gf16_ptrs_stream_kernel<W, 5>)
        const void* pk[] = {KP_(2), KP_(4), KP_(8)};
#undef KP_
        for (const void* k : pk)
            HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
#define KFN_(W, MB) reinterpret_cast<const void*>(&gf16_frame_crc_kernel<W, 1, MB, true>),     \
               reinterpret_cast<const void*>(&gf16_frame_crc_kernel<W, 2, MB, true>),         \
               reinterpret_cast<const void*>(&gf16_frame_crc_kernel<W, 3, MB, true>),         \
               reinterpret_cast<const void*>(&gf16_frame_crc_kernel<W, 4, MB, true>),         \
               reinterpret_cast<const void*>(&gf16_frame_crc_kernel<W, 5, MB, true>)
#define KF_(W, MB) reinterpret_cast<const void*>(&gf16_frame_crc_kernel<W, 1, MB>),           \
               reinterpret_cast<const void*>(&gf16_frame_crc_kernel<W, 2, MB>),               \
               reinterpret_cast<const void*>(&gf16_frame_crc_kernel<W, 3, MB>),               \
               reinterpret_cast<const void*>(&gf16_frame_crc_kernel<W, 4, MB>),               \
               reinterpret_cast<const void*>(&gf16_frame_crc_kernel<W, 5, MB>)
        const void* fk[] = {KF_(2, 1), KF_(4, 1), KF_(8, 1), KF_(2, 4), KF_(4, 4), KF_(8, 4),
                            KFN_(2, 4), KFN_(4, 4), KFN_(8, 4), KFN_(2, 1), KFN_(4, 1), KFN_(8, 1),
                            reinterpret_cast<const void*>(&gf16_hybrid_kernel<1>),
                            reinterpret_cast<const void*>(&gf16_hybrid_kernel<2>),
                            reinterpret_cast<const void*>(&gf16_hybrid_kernel<3>),
                            reinterpret_cast<const void*>(&gf16_hybrid_kernel<4>),
                            reinterpret_cast<const void*>(&gf16_hybrid_kernel<5>),
#define KR_(W) reinterpret_cast<const void*>(&gf16_realign_kernel<W, 1>),                        \
               reinterpret_cast<const void*>(&gf16_realign_kernel<W, 2>),                        \
               reinterpret_cast<const void*>(&gf16_realign_kernel<W, 3>),                        \
               reinterpret_cast<const void*>(&gf16_realign_kernel<W, 4>),                        \
               reinterpret_cast<const void*>(&gf16_realign_kernel<W, 5>)
                            KR_(2), KR_(4)};
#undef KR_
#undef KF_
#undef KFN_
        for (const void* k : fk)
            HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
        for (const void* k : sk)
            HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
        di.lds_attr_set = true;
    }
    if (dev_out) *dev_out = dev;
    return 0;
}

int cu_count(int dev)
{
    std::lock_guard<std::mutex> lk(g_dev_mu);
    return g_dev[dev].cus;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

namespace ecamd {

int dev_ensure(int* dev_out) { return ensure_device(dev_out); }
int dev_cu_count(int dev) { return cu_count(dev); }
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

int launch_stripes(int nstripes, uint64_t tiles_per_stripe, uint64_t slots, uint64_t limit)
{
    const uint64_t ntiles = tiles_per_stripe * static_cast<uint64_t>(nstripes);
    if (!limit || ntiles <= limit * slots) return nstripes;
    const uint64_t launches = (ntiles + limit * slots - 1) / (limit * slots);
    return static_cast<int>((static_cast<uint64_t>(nstripes) + launches - 1) / launches);
}

}  // namespace ecamd

struct ecamd_map {
    struct Pass {
        int row0, width, col0, ncols;
        size_t offset;  // into d_tables: byte-split image
        size_t bytes;
        size_t nib_offset;  // nibble image (build_nibble_tables)
        size_t nib_bytes;
    };
    int device = 0;
    int R = 0, K = 0;
    std::vector<Pass> passes;
    uint8_t* d_tables = nullptr;
    std::vector<int> coeff;  // R x K (host copy: the bitsliced kernels are generated from it)
    // this map's identity for whatever caches its tables (the resident small server's slots): from a
    // process-wide counter at creation, never reused -- d_tables' address is, once the map is destroyed
    uint64_t serial = 0;
};

namespace ecamd {
hipFunction_t bitslice_function(int dev, const std::vector<int>& coeff, int R, int K, int depth, bool wait,
                                std::shared_ptr<void>& hold, bool copy = false, int crc = 0, bool wave = false,
                                const std::vector<int>* in_shift = nullptr, int prefetch = 0, int* status = nullptr,
                                const BsOcc* occ = nullptr, bool check = false, bool locate = false, int opts = 0);
int bitslice_prebuild(const std::vector<int>& coeff, int R, int K, int depth, bool copy, int crc, bool wave,
                      const std::vector<int>* in_shift, int prefetch, const BsOcc& occ, const std::string& arch,
                      const std::string& dir, bool check = false, bool locate = false, int opts = 0);
int bitslice_launch(hipFunction_t fn, const BsArgs& args, int grid, hipStream_t st,
                    const std::shared_ptr<void>& hold, int threads = 256, unsigned lds = 0);
}  // namespace ecamd

namespace {

// Row groups of width 2/4/8 and column chunks that fit the LDS of one workgroup.
std::vector<ecamd_map::Pass> plan_passes(int R, int K)
{
    int width;
    if (R <= 2)
        width = 2;
    else if (R <= 4)
        width = 4;
    else
        width = (K <= kLdsBytes / (512 * 16)) ? 8 : 4;
    const int maxcols = std::min(kMaxCols, kLdsBytes / (512 * 2 * width));
    std::vector<ecamd_map::Pass> passes;
    size_t off = 0;
    for (int row0 = 0; row0 < R; row0 += width) {
        for (int col0 = 0; col0 < K; col0 += maxcols) {
            ecamd_map::Pass p;
            p.row0 = row0;
            p.width = width;
            p.col0 = col0;
            p.ncols = std::min(maxcols, K - col0);
            p.offset = off;
            p.bytes = static_cast<size_t>(p.ncols) * 512 * 2 * width;
            off += p.bytes;
            passes.push_back(p);
        }
    }
    return passes;
}

struct Geometry {
    int threads;
    int grid;
    size_t lds;
    uint32_t tiles_per_stripe;
    uint32_t ntiles;
};

int geometry(int dev, size_t lds, int64_t bs, int nstripes, Geometry& g, int chunks = 1,
             int max_threads = 1024, int max_wgs = 8, int grid_mult = 1)
{
    int wgs = lds ? static_cast<int>(std::min<size_t>(max_wgs, std::max<size_t>(1, kLdsBytes / lds))) : 8;
    int threads = lds ? std::min(1024, std::max(256, (1024 / wgs) / 64 * 64)) : 256;
    if (lds && g_tune.threads > 0) threads = g_tune.threads;
    threads = std::min(threads, max_threads);
    if (lds && g_tune.wgs_per_cu > 0) wgs = std::min<int>(g_tune.wgs_per_cu, std::max<size_t>(1, kLdsBytes / lds));
    int64_t span = static_cast<int64_t>(threads) * 16 * chunks;
    int64_t tps = (bs + span - 1) / span;
    int64_t nt = tps * nstripes;
    if (nt >= (1ll << 32)) return fail(ECAMD_EINVAL, "batch too large: %lld tiles", (long long)nt);
    g.threads = threads;
    g.lds = lds;
    g.tiles_per_stripe = static_cast<uint32_t>(tps);
    g.ntiles = static_cast<uint32_t>(nt);
    int64_t grid = std::min<int64_t>(nt, static_cast<int64_t>(cu_count(dev)) * wgs * std::max(1, grid_mult));
    g.grid = static_cast<int>(std::max<int64_t>(grid, 1));
    return 0;
}

// gf16_stream_kernel addresses a stripe's fragments as 32-bit offsets from one buffer resource:
// usable when every offset is non-negative and the furthest byte stays below 2^31.
bool stream_offsets(ApplyArgs& a, int64_t bs)
{
    int64_t in_max = 0, out_max = 0;
    for (int j = 0; j < a.ncols; j++) {
        if (a.in_off[j] < 0) return false;
        in_max = std::max(in_max, a.in_off[j] + bs);
    }
    for (int r = 0; r < a.nrows; r++) {
        if (a.out_off[r] < 0) return false;
        out_max = std::max(out_max, a.out_off[r] + bs);
    }
    const int64_t lim = int64_t(1) << 31;
    if (in_max >= lim || out_max >= lim) return false;
    for (int j = 0; j < a.ncols; j++) a.in_off32[j] = static_cast<int32_t>(a.in_off[j]);
    for (int r = 0; r < a.nrows; r++) a.out_off32[r] = static_cast<int32_t>(a.out_off[r]);
    a.in_records = static_cast<uint32_t>(in_max);
    a.out_records = static_cast<uint32_t>(out_max);
    return true;
}

// Copy-through offsets for gf16_stream_kernel (framed encode / decode-join): every non-skipped
// copy destination must be addressable as a 32-bit offset from the stripe's copy_base.
bool stream_copy_offsets(ApplyArgs& a, int64_t bs)
{
    int64_t mx = 0;
    for (int j = 0; j < a.ncols; j++) {
        if (a.copy_off[j] < 0) continue;
        mx = std::max(mx, a.copy_off[j] + bs);
    }
    if (mx >= (int64_t(1) << 31)) return false;
    for (int j = 0; j < a.ncols; j++)
        a.copy_off32[j] = a.copy_off[j] < 0 ? -1 : static_cast<int32_t>(a.copy_off[j]);
    a.copy_records = static_cast<uint32_t>(std::max<int64_t>(mx, 16));
    return true;
}

// A pass small enough for gf16_small_kernel: at most small_chunks 16-byte chunks in all, plain
// strided fragments (no copy-through, padding limits or stripe list) at one 16-byte aligned pitch
// per side.
bool small_launch(const ApplyArgs& a, int64_t bs, int nstripes)
{
    const int64_t chunks = (bs + 15) / 16 * nstripes;
    if (chunks <= 0 || chunks > g_tune.small_chunks || a.limited || a.copy_base || a.stripe_list ||
        a.ncols < 1 || a.nrows < 1)
        return false;
    auto uniform = [nstripes](const uint8_t* base, int64_t stride, const int64_t* off, int n) {
        const int64_t pitch = n > 1 ? off[1] - off[0] : 16;
        for (int j = 0; j < n; j++)
            if (off[j] != off[0] + j * pitch) return false;
        return ((reinterpret_cast<uintptr_t>(base) + off[0]) & 15) == 0 && (pitch & 15) == 0 &&
               (nstripes == 1 || (stride & 15) == 0);
    };
    return uniform(a.in_base, a.in_stride, a.in_off, a.ncols) &&
           uniform(a.out_base, a.out_stride, a.out_off, a.nrows);
}

SmallArgs small_args(const ApplyArgs& a, int64_t bs, int nstripes, int lane)
{
    SmallArgs s{};
    s.in = a.in_base + a.in_off[0];
    s.out = a.out_base + a.out_off[0];
    s.in_stride = a.in_stride;
    s.out_stride = a.out_stride;
    s.in_pitch = a.ncols > 1 ? a.in_off[1] - a.in_off[0] : 0;
    s.out_pitch = a.nrows > 1 ? a.out_off[1] - a.out_off[0] : 0;
    s.bs = bs;
    s.cpf = (bs + lane - 1) / lane;
    s.nchunks = s.cpf * nstripes;
    s.ncols = a.ncols;
    s.nrows = a.nrows;
    s.accumulate = a.accumulate;
    for (int r = 0; r < kMaxRows; r++) s.masks[r] = r < a.nrows ? a.masks[r] : 0u;
    return s;
}

// The fused checksum of a small launch (gf16_small_kernel CRC): the device image, where the CRCs go,
// the partials' scratch and the machine.
struct SmallCrcReq {
    const uint32_t* img[2];  // build_small_crc_image for 2- and 4-byte lanes
    uint32_t* out;
    uint32_t* part;
    bool legacy;
};

// The calling thread's armed completion flag (ecamd_done_flag_arm): taken by its next small launch that
// ends an operation.
struct DoneFlag {
    uint32_t* flag = nullptr;
    uint32_t value = 0;
    bool taken = false;
    // the resident small server (ecamd_done_flag_arm_server): 1 any small launch that is the whole
    // operation may be posted to it, 2 only a fused-checksum one; served: it was
    int server = 0;
    bool served = false;
};
thread_local DoneFlag t_done;

// Attaches the thread's armed completion flag to a small launch of `grid` workgroups that ends its
// operation: several workgroups count in the stream's scratch slot (its context held in `use` until the
// launch is enqueued, so it is not released meanwhile); a fused checksum counts with its own counter.
void attach_done(SmallArgs& s, unsigned grid, bool crc, hipStream_t st, std::unique_ptr<StreamUse>& use)
{
    if (!t_done.flag || t_done.taken) return;
    if (grid > 1 && !crc) {
        int dev = 0;
        uint32_t* scr = nullptr;
        if (hipGetDevice(&dev) == hipSuccess) {
            use = std::make_unique<StreamUse>(dev, st);
            if (stream_scratch(dev, st, kSmallCrcScratchSlot, 16, &scr) == 0) s.done_ctr = scr + 1;
        }
        (void)hipGetLastError();
    }
    if (grid == 1 || crc || s.done_ctr) {
        s.done = t_done.flag;
        s.done_val = t_done.value;
    }
}

// ---- The resident small server (small_server_kernel) ----
// A per-call operation that is ONE small launch -- its inputs and outputs in the pinned slab, nothing else
// on its stream -- is posted to a mailbox instead of launched: the caller thread's server (kSmallServerWgs
// workgroups of one (W, G) or XOR, with and without the fused checksum, on a stream of its own; another
// key stops it and launches that one) polls it, runs the same body, and
// stores the same completion flag.  Host-side launch latency (~3-4 us of hipLaunchKernel) and the kernel's
// start (~5 us) leave the call; the mailbox round trip is ~4 us (tools/mailbox_probe.py).  A request with
// the previous one's arguments (but the flag value) is posted without them: the server reuses its copy and
// the tables it staged.  The server exits idle_us after its last request or on stop (thread exit); a post after its exit is noticed
// by ecamd_small_server_wait, which relaunches it with the request pending (that server skips it if its
// flag is already set).  Its counters and checksum partials are its own scratch, zeroed at creation.
struct SmallServer {
    int dev = -1;
    hipStream_t st = nullptr;
    SmallServerBox* box = nullptr;  // coherent pinned host memory
    uint32_t* scratch = nullptr;    // device: word 1 the done counter, from word 64 the checksum partials
    uint32_t key = 0;  // of the launched kernel: W | G << 4, or kSmallServerXor
    uint32_t post = 0, prev = 0, seq = 0;
    bool running = false;
    ServerSlotEntry<SmallArgs> cached[2];  // box slot i holds cached[i].args (this server instance)
    uint32_t gen[2] = {0, 0};  // slot generations (8 bits in the post word)
    int last_slot = 0;
    std::chrono::steady_clock::time_point last{};
};
constexpr size_t kServerScratchWords = 64 + 16 + 64 * kSmallServerWgs;  // partials: 16 + (K + R) * workgroups
constexpr int kMaxSmallServers = 8;
constexpr size_t kServerLds = kLdsBytes - 1024;  // the server's dynamic LDS (its static share is < 1 KiB)
static_assert(2 * static_cast<size_t>(kSmallServerLdsHalf) <= kServerLds, "two table placements");
std::mutex g_srv_mu;
auto& g_srv_free = *new std::vector<SmallServer*>();  // idle servers of exited threads (never freed)
std::atomic<long long> g_srv_posts{0}, g_srv_launches{0}, g_srv_rewrites{0}, g_srv_stale_hits{0};
int g_srv_count = 0;

// ECAMD_PERCALL_SERVER_IDLE_US: how long a server polls without a request (default 2000 us)
int64_t server_idle_us()
{
    static const int64_t v = [] {
        const char* e = std::getenv("ECAMD_PERCALL_SERVER_IDLE_US");
        const long long x = e ? std::atoll(e) : 2000;
        return static_cast<int64_t>(std::clamp<long long>(x, 50, 1000000));
    }();
    return v;
}

struct ServerHold {
    SmallServer* s = nullptr;
    ~ServerHold()
    {
        if (!s) return;
        __atomic_store_n(&s->box->stop, 1u, __ATOMIC_RELEASE);  // its workgroups exit at their next poll
        std::lock_guard<std::mutex> lk(g_srv_mu);
        g_srv_free.push_back(s);
    }
};
thread_local ServerHold t_srv;

SmallServer* thread_server(int dev)
{
    if (t_srv.s) return t_srv.s->dev == dev ? t_srv.s : nullptr;
    std::unique_lock<std::mutex> lk(g_srv_mu);
    for (size_t i = 0; i < g_srv_free.size(); i++) {
        SmallServer* sv = g_srv_free[i];
        if (sv->dev != dev) continue;
        g_srv_free.erase(g_srv_free.begin() + static_cast<std::ptrdiff_t>(i));
        lk.unlock();
        if (hipStreamSynchronize(sv->st) != hipSuccess) {  // its kernel saw stop
            (void)hipGetLastError();
            return nullptr;
        }
        __atomic_store_n(&sv->box->stop, 0u, __ATOMIC_RELEASE);
        sv->running = false;
        t_srv.s = sv;
        return sv;
    }
    if (g_srv_count >= kMaxSmallServers) return nullptr;
    g_srv_count++;
    lk.unlock();
    auto sv = std::make_unique<SmallServer>();
    sv->dev = dev;
    bool ok = hipHostMalloc(reinterpret_cast<void**>(&sv->box), sizeof(SmallServerBox), hipHostMallocDefault) ==
              hipSuccess;
    ok = ok && hipMalloc(&sv->scratch, kServerScratchWords * 4) == hipSuccess &&
         hipMemset(sv->scratch, 0, kServerScratchWords * 4) == hipSuccess &&
         hipStreamCreateWithFlags(&sv->st, hipStreamNonBlocking) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        if (sv->box) (void)hipHostFree(sv->box);
        if (sv->scratch) (void)hipFree(sv->scratch);
        std::lock_guard<std::mutex> lk2(g_srv_mu);
        g_srv_count--;
        return nullptr;
    }
    std::memset(sv->box, 0, sizeof(SmallServerBox));
    t_srv.s = sv.release();
    return t_srv.s;
}

int server_launch(SmallServer* sv, uint32_t key, uint32_t post0, bool dup)
{
    SmallServerArgs a{sv->box, post0, dup ? 1u : 0u, static_cast<uint64_t>(server_idle_us()) * 100u};
    const void* k = nullptr;
    switch (key) {
#define SV_(V)                                                              \
    case (V): k = reinterpret_cast<const void*>(&small_server_kernel<(V)>); \
        break;
        SV_(2 | (2 << 4)) SV_(4 | (2 << 4)) SV_(8 | (2 << 4)) SV_(2 | (4 << 4)) SV_(4 | (4 << 4)) SV_(8 | (4 << 4))
        SV_(kSmallServerXor)
#undef SV_
    default: return fail(ECAMD_EINVAL, "small server key %u", key);
    }
    HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kServerLds)));
    void* args[] = {&a};
    HIP_TRY(hipLaunchKernel(k, dim3(kSmallServerWgs), dim3(256), args, kServerLds, sv->st));
    sv->running = true;
    sv->key = key;
    g_srv_launches.fetch_add(1, std::memory_order_relaxed);
    return 0;
}

// Posts the small launch `s` (variant, nblk workgroups, lds bytes) to the calling thread's server: 0 posted,
// 1 not taken (the caller launches it), < 0 an error.  `serial`: of the map s.tables belongs to (0: no tables).
int server_post(SmallArgs& s, uint32_t variant, uint64_t serial, unsigned nblk, size_t lds, bool crc)
{
    if (nblk == 0 || nblk > static_cast<unsigned>(kSmallServerWgs) || lds > kServerLds) return 1;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return 1;
    }
    SmallServer* sv = thread_server(dev);
    if (!sv) return 1;
    s.done_ctr = sv->scratch + 1;
    if (crc) s.crc_part = sv->scratch + 64;
    const auto now = std::chrono::steady_clock::now();
    const uint32_t key = variant & ~256u;  // the checksum form runs in the same kernel
    bool launch = !sv->running || sv->key != key;
    if (!launch && now - sv->last > std::chrono::microseconds(server_idle_us() / 2)) {
        const hipError_t q = hipStreamQuery(sv->st);  // past half its idle time: did it exit?
        if (q == hipSuccess)
            launch = true;
        else if (q != hipErrorNotReady)
            return fail(ECAMD_EHIP, "small server: %s", hipGetErrorString(q));
    }
    if (launch) {
        if (sv->running && sv->key != key) {  // another kernel: stop this one first
            __atomic_store_n(&sv->box->stop, 1u, __ATOMIC_RELEASE);
            HIP_TRY(hipStreamSynchronize(sv->st));
            __atomic_store_n(&sv->box->stop, 0u, __ATOMIC_RELEASE);
        }
        const int rc = server_launch(sv, key, sv->post, false);
        if (rc) return rc;
    }
    // a cached request's arguments but for the flag value, of the same map (the common case: one caller
    // repeating one operation, or alternating two, on one size): the slot is not rewritten and the server
    // keeps its copy (and its staged tables when they are that slot's) -- server_slot_choose
    if (launch) sv->cached[0].have = sv->cached[1].have = false;  // (a new instance holds no block: new generations)
    const ServerSlotChoice ch = server_slot_choose(s, variant, serial, sv->cached, sv->last_slot);
    const int slot = ch.slot;
    if (ch.stale) g_srv_stale_hits.fetch_add(1, std::memory_order_relaxed);
    if (ch.rewrite) {  // the slot not used last
        std::memcpy(&sv->box->slot[slot].args, &s, sizeof(SmallArgs));
        sv->box->variant[slot] = variant;
        sv->gen[slot] = (sv->gen[slot] + 1u) & 0xffu;
        g_srv_rewrites.fetch_add(1, std::memory_order_relaxed);
    }
    server_slot_note(ch, s, variant, serial, sv->cached, sv->last_slot);
    sv->seq = sv->seq % 0x3fffu + 1u;
    sv->prev = sv->post;
    sv->post = (sv->seq << 18) | (sv->gen[slot] << 10) | (slot ? kSmallServerSlot : 0u) |
               (lds <= static_cast<size_t>(kSmallServerLdsHalf) ? kSmallServerHalf : 0u) | nblk;
    __atomic_store_n(&sv->box->done_val, s.done_val, __ATOMIC_RELAXED);
    __atomic_store_n(&sv->box->post, sv->post, __ATOMIC_RELEASE);  // after the rest (x86: stores in order)
    sv->last = now;
    g_srv_posts.fetch_add(1, std::memory_order_relaxed);
    return 0;
}

// Whether a small launch may go to the server: armed for it, the whole operation, staged inputs.
bool server_wanted(bool crc, bool only, bool st_in, int nstripes, const SmallArgs& s)
{
    return only && st_in && nstripes == 1 && s.done && !t_done.taken &&
           (t_done.server == 1 || (t_done.server == 2 && crc));
}

// ECAMD_EINVAL (nothing launched) when `crc` is given and the launch cannot fuse it.  `last`: this launch
// ends the operation (the completion flag may be attached to it); `only`: it is the whole operation (then
// it may be posted to the resident small server).
int launch_small(const ApplyArgs& a, const ecamd_map::Pass& p, int64_t bs, int nstripes, const uint8_t* tables,
                 uint64_t serial, hipStream_t st, const SmallCrcReq* crc = nullptr, bool last = false,
                 bool only = false)
{
    const int lane = g_tune.small_lane ? static_cast<int>(g_tune.small_lane)
                                       : ((bs + 1) / 2 * nstripes <= 256 ? 2 : 4);
    const int width = p.width;
    SmallArgs s = small_args(a, bs, nstripes, lane);
    s.tables = tables + p.offset;
    const dim3 grid(static_cast<unsigned>((s.nchunks + 255) / 256)), block(256);
    // staged inputs (gf16_small_kernel ST): one stripe, inputs at a 16-byte pitch from a 16-byte
    // aligned base, the workgroup's 256 * lane bytes of every input beside the tables in LDS
    const size_t stage = static_cast<size_t>(crc ? a.ncols + a.nrows : a.ncols) * 256 * lane +
                         (crc ? static_cast<size_t>(small_crc_words(lane)) * 4 : 0);
    const bool st_in = (g_tune.small_stage || crc) && nstripes == 1 && (s.in_pitch % 16) == 0 && aligned16(s.in) &&
                       p.bytes + stage <= kLdsBytes &&
                       (a.ncols - 1) * s.in_pitch + bs < (int64_t(1) << 31);
    const size_t lds = p.bytes + (st_in ? stage : 0);
    std::unique_ptr<StreamUse> use;
    if (last) attach_done(s, grid.x, crc != nullptr, st, use);
    if (crc) {
        // the region-shift maps reach 63 regions past a workgroup's: at most 64 workgroups
        if (!st_in || (lane != 2 && lane != 4) || a.accumulate || grid.x > 64) return ECAMD_EINVAL;
        s.crc_img = crc->img[lane == 2 ? 0 : 1];
        const SmallCrcConst k = small_crc_const(crc->legacy, static_cast<uint64_t>(bs),
                                                static_cast<uint64_t>(grid.x) * 256 * lane - static_cast<uint64_t>(bs));
        s.crc_out = crc->out;
        s.crc_dbg = static_cast<int>(g_tune.small_crc_dbg);
        s.crc_part = crc->part;
        std::copy(k.minv, k.minv + 32, s.crc_minv);
        s.crc_c = k.c;
        if (server_wanted(true, only, st_in, nstripes, s)) {
            const int r = server_post(s, static_cast<uint32_t>(width | (lane << 4) | 256), serial, grid.x, lds, true);
            if (r < 0) return r;
            if (r == 0) {
                t_done.taken = t_done.served = true;
                return 0;
            }
        }
#define SMALLC_(W)                                                                                          \
    if (lane == 2)                                                                                          \
        hipLaunchKernelGGL((gf16_small_kernel<W, 2, true, true>), grid, block, lds, st, s);                 \
    else                                                                                                    \
        hipLaunchKernelGGL((gf16_small_kernel<W, 4, true, true>), grid, block, lds, st, s);
        if (width == 2) {
            SMALLC_(2)
        } else if (width == 4) {
            SMALLC_(4)
        } else {
            SMALLC_(8)
        }
#undef SMALLC_
        HIP_TRY(hipGetLastError());
        if (s.done) t_done.taken = true;
        return 0;
    }
    if ((lane == 2 || lane == 4) && server_wanted(false, only, st_in, nstripes, s)) {
        const int r = server_post(s, static_cast<uint32_t>(width | (lane << 4)), serial, grid.x, lds, false);
        if (r < 0) return r;
        if (r == 0) {
            t_done.taken = t_done.served = true;
            return 0;
        }
    }
#define SMALL_(W)                                                                                           \
    switch (lane * 2 + (st_in ? 1 : 0)) {                                                                   \
    case 4: hipLaunchKernelGGL((gf16_small_kernel<W, 2, false>), grid, block, lds, st, s); break;          \
    case 5: hipLaunchKernelGGL((gf16_small_kernel<W, 2, true>), grid, block, lds, st, s); break;           \
    case 32: hipLaunchKernelGGL((gf16_small_kernel<W, 16, false>), grid, block, lds, st, s); break;        \
    case 33: hipLaunchKernelGGL((gf16_small_kernel<W, 16, true>), grid, block, lds, st, s); break;         \
    case 9: hipLaunchKernelGGL((gf16_small_kernel<W, 4, true>), grid, block, lds, st, s); break;           \
    default: hipLaunchKernelGGL((gf16_small_kernel<W, 4, false>), grid, block, lds, st, s); break;         \
    }
    if (width == 2) {
        SMALL_(2)
    } else if (width == 4) {
        SMALL_(4)
    } else {
        SMALL_(8)
    }
#undef SMALL_
    HIP_TRY(hipGetLastError());
    if (s.done) t_done.taken = true;
    return 0;
}

// `last`: this launch ends the operation (the completion flag may be attached).  ECAMD_EINVAL (nothing
// launched) when `crc` is given and the launch cannot fuse it.
int launch_xor_small(const ApplyArgs& a, int64_t bs, int nstripes, hipStream_t st, bool last = false,
                     const SmallCrcReq* crc = nullptr, bool only = false)
{
    SmallArgs s = small_args(a, bs, nstripes, 4);
    const unsigned grid = static_cast<unsigned>((s.nchunks + 255) / 256);
    // staged inputs (xor_small_kernel ST), as launch_small: one stripe, a 16-byte pitch and base, 1 KiB per input
    const bool st_in = (g_tune.small_stage || crc) && nstripes == 1 && (s.in_pitch % 16) == 0 && aligned16(s.in) &&
                       (a.ncols - 1) * s.in_pitch + bs < (int64_t(1) << 31);
    if (crc) {
        if (!st_in || a.accumulate || grid > 64) return ECAMD_EINVAL;
        const SmallCrcConst k = small_crc_const(crc->legacy, static_cast<uint64_t>(bs),
                                                static_cast<uint64_t>(grid) * 1024 - static_cast<uint64_t>(bs));
        s.crc_img = crc->img[1];
        s.crc_out = crc->out;
        s.crc_part = crc->part;
        std::copy(k.minv, k.minv + 32, s.crc_minv);
        s.crc_c = k.c;
    }
    std::unique_ptr<StreamUse> use;
    if (last) attach_done(s, grid, crc != nullptr, st, use);
    const size_t stage = static_cast<size_t>(crc ? a.ncols + a.nrows : a.ncols) * 1024 +
                         (crc ? static_cast<size_t>(small_crc_words(4)) * 4 : 0);
    if (server_wanted(crc != nullptr, only, st_in, nstripes, s)) {
        const int r = server_post(s, kSmallServerXor | (crc ? 256u : 0u), 0, grid, stage, crc != nullptr);
        if (r < 0) return r;
        if (r == 0) {
            t_done.taken = t_done.served = true;
            return 0;
        }
    }
    if (crc)
        hipLaunchKernelGGL((xor_small_kernel<true, true>), dim3(grid), dim3(256), stage, st, s);
    else if (st_in)
        hipLaunchKernelGGL((xor_small_kernel<true, false>), dim3(grid), dim3(256), stage, st, s);
    else
        hipLaunchKernelGGL((xor_small_kernel<false, false>), dim3(grid), dim3(256), 0, st, s);
    HIP_TRY(hipGetLastError());
    if (s.done) t_done.taken = true;
    return 0;
}

template <int W, int CH, bool PF, bool NIB = false>
int launch_stream_w(const ApplyArgs& a, dim3 grid, dim3 block, size_t lds, hipStream_t st)
{
    const int kg = (a.ncols + 3) / 4;
    switch (kg) {
    case 1: hipLaunchKernelGGL((gf16_stream_kernel<W, 1, CH, PF, NIB>), grid, block, lds, st, a); break;
    case 2: hipLaunchKernelGGL((gf16_stream_kernel<W, 2, CH, PF, NIB>), grid, block, lds, st, a); break;
    case 3: hipLaunchKernelGGL((gf16_stream_kernel<W, 3, CH, PF, NIB>), grid, block, lds, st, a); break;
    case 4: hipLaunchKernelGGL((gf16_stream_kernel<W, 4, CH, PF, NIB>), grid, block, lds, st, a); break;
    default: hipLaunchKernelGGL((gf16_stream_kernel<W, 5, CH, PF, NIB>), grid, block, lds, st, a); break;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_stream(const ApplyArgs& a, int width, int ch, bool pf, bool nib, dim3 grid, dim3 block,
                  size_t lds, hipStream_t st)
{
    bool unaligned = false;  // inputs at offsets that are not multiples of 16 (objects, j*bs)
    for (int j = 0; j < a.ncols; j++) unaligned = unaligned || (a.in_off32[j] & 15) != 0;
    if (unaligned && width <= 4 && ch == 1 && !nib && g_tune.stream_realign) {
        ApplyArgs ra = a;
        ra.realign_dpp = g_tune.stream_realign == 2 ? 1 : 0;
        // aligned loads realigned in registers (ecamd_stream.hpp, RA)
#define RA_(W)                                                                                    \
    switch ((a.ncols + 3) / 4) {                                                                  \
    case 1: hipLaunchKernelGGL((gf16_realign_kernel<W, 1>), grid, block, lds, st, ra); break;      \
    case 2: hipLaunchKernelGGL((gf16_realign_kernel<W, 2>), grid, block, lds, st, ra); break;      \
    case 3: hipLaunchKernelGGL((gf16_realign_kernel<W, 3>), grid, block, lds, st, ra); break;      \
    case 4: hipLaunchKernelGGL((gf16_realign_kernel<W, 4>), grid, block, lds, st, ra); break;      \
    default: hipLaunchKernelGGL((gf16_realign_kernel<W, 5>), grid, block, lds, st, ra); break;     \
    }
        if (width == 2) {
            RA_(2)
        } else {
            RA_(4)
        }
#undef RA_
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (width == 8 && !nib && g_tune.stream_hybrid) {  // LDS + L1 lookups (gf16_hybrid_kernel)
        switch ((a.ncols + 3) / 4) {
        case 1: hipLaunchKernelGGL((gf16_hybrid_kernel<1>), grid, block, lds, st, a); break;
        case 2: hipLaunchKernelGGL((gf16_hybrid_kernel<2>), grid, block, lds, st, a); break;
        case 3: hipLaunchKernelGGL((gf16_hybrid_kernel<3>), grid, block, lds, st, a); break;
        case 4: hipLaunchKernelGGL((gf16_hybrid_kernel<4>), grid, block, lds, st, a); break;
        default: hipLaunchKernelGGL((gf16_hybrid_kernel<5>), grid, block, lds, st, a); break;
        }
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (nib) {  // a.tables is the nibble image
        if (width == 2) return launch_stream_w<2, 1, false, true>(a, grid, block, lds, st);
        if (width == 4) return launch_stream_w<4, 1, false, true>(a, grid, block, lds, st);
        return launch_stream_w<8, 1, false, true>(a, grid, block, lds, st);
    }
    if (ch == 2 && width <= 4) {
        if (pf)
            return width == 2 ? launch_stream_w<2, 2, true>(a, grid, block, lds, st)
                              : launch_stream_w<4, 2, true>(a, grid, block, lds, st);
        return width == 2 ? launch_stream_w<2, 2, false>(a, grid, block, lds, st)
                          : launch_stream_w<4, 2, false>(a, grid, block, lds, st);
    }
    if (pf) {
        if (width == 2) return launch_stream_w<2, 1, true>(a, grid, block, lds, st);
        if (width == 4) return launch_stream_w<4, 1, true>(a, grid, block, lds, st);
        return launch_stream_w<8, 1, true>(a, grid, block, lds, st);
    }
    if (width == 2) return launch_stream_w<2, 1, false>(a, grid, block, lds, st);
    if (width == 4) return launch_stream_w<4, 1, false>(a, grid, block, lds, st);
    return launch_stream_w<8, 1, false>(a, grid, block, lds, st);
}

// One strided stream pass over a batch.  Within one launch the workgroups drift apart as they go
// and the tiles in flight spread over more and more of the batch, which costs HBM rate (C3, 2048
// stripes: one launch 5.34 TB/s, launches of 32 tiles per resident workgroup 5.85; 256 stripes
// spread over the span of 2048: 5.06-5.22, tools/span_probe.py, tools/slot_sweep.py,
// profiles/r02_{span_probe,slot_sweep}.log).  So a pass runs as launches of at most tiles_per_slot
// tiles per resident workgroup -- 32 for 4-output passes (C3 256 stripes: two launches, 0-2%
// faster than one), 64 for the others (C2 loses 1.5% at 32: its launches are short) -- each
// starting its workgroups in step again; 4-output launches of at most 64 tiles per slot take
// twice the resident workgroups (C3 +1.2-2.7%; C2 -7% and C5 -2-4% that way, so only there).
// The stripe ranges of a strided pass split into launches of at most `limit` tiles per resident
// workgroup (`slots` of them), as even as the stripes allow; launch(args, stripes) per range, the
// args' bases (or stripe list) moved to the range's first stripe.
template <class Launch>
int for_each_launch(const ApplyArgs& a, int nstripes, uint64_t tiles_per_stripe, uint64_t slots,
                    uint64_t limit, Launch&& launch)
{
    const int per = launch_stripes(nstripes, tiles_per_stripe, slots, limit);
    for (int s0 = 0; s0 < nstripes; s0 += per) {
        ApplyArgs c = a;
        if (a.stripe_list) {
            c.stripe_list = a.stripe_list + s0;  // stripe indices stay absolute
        } else {
            c.in_base = a.in_base + s0 * a.in_stride;
            c.out_base = a.out_base + s0 * a.out_stride;
            if (a.copy_records) c.copy_base = a.copy_base + s0 * a.copy_stride;
        }
        const int rc = launch(c, std::min(per, nstripes - s0));
        if (rc) return rc;
    }
    return 0;
}

// True when the output fragments of a pass are one run of consecutive slots (an encode's parity, a
// decode of adjacent fragments) -- the write pattern the 2-tile ranges suit.  The slot spacing is the
// smallest distance between any two fragments the pass touches (inputs and outputs) when both live
// in one layout; a copy-through pass reads objects (in_base != out_base), so its inputs count by the
// payload slots they are copied to when those share the outputs' layout, else only its outputs.
bool outputs_consecutive(const ApplyArgs& a, int64_t bs)
{
    if (a.nrows <= 1) return true;
    std::vector<int64_t> offs;
    if (a.in_base == a.out_base && a.in_stride == a.out_stride)
        for (int j = 0; j < a.ncols; j++) offs.push_back(a.in_off[j]);
    else if (a.copy_records && a.copy_base == a.out_base && a.copy_stride == a.out_stride)
        for (int j = 0; j < a.ncols; j++)  // the inputs' payload slots, beside the outputs
            if (a.copy_off[j] >= 0) offs.push_back(a.copy_off[j]);
    for (int r = 0; r < a.nrows; r++) offs.push_back(a.out_off[r]);
    std::sort(offs.begin(), offs.end());
    int64_t slot = INT64_MAX;
    for (size_t i = 1; i < offs.size(); i++)
        if (offs[i] > offs[i - 1]) slot = std::min(slot, offs[i] - offs[i - 1]);
    if (slot == INT64_MAX || slot < bs) return false;
    int64_t lo = a.out_off[0], hi = a.out_off[0];
    for (int r = 1; r < a.nrows; r++) {
        lo = std::min(lo, a.out_off[r]);
        hi = std::max(hi, a.out_off[r]);
    }
    return hi - lo == slot * (a.nrows - 1);
}

int launch_stream_pass(ApplyArgs a, int dev, size_t lds_bytes, int width, int ch, bool nib,
                       int64_t bs, int nstripes, hipStream_t st)
{
    const int knob = g_tune.tiles_per_slot;
    const uint64_t limit = knob > 0 ? static_cast<uint64_t>(knob) : (width == 4 ? 32 : 64);
    Geometry g;
    int rc = geometry(dev, lds_bytes, bs, nstripes, g, ch, 1024, 4, 1);
    if (rc) return rc;
    return for_each_launch(a, nstripes, g.tiles_per_stripe, g.grid, limit, [&](ApplyArgs& c, int n) {
        Geometry h;
        int r = geometry(dev, lds_bytes, bs, n, h, ch, 1024, 4, 1);
        if (r) return r;
        const int gm = g_tune.grid_mult > 0 ? g_tune.grid_mult
                                            : (width == 4 && h.ntiles <= 64ull * h.grid ? 2 : 1);
        if (gm != 1 && (r = geometry(dev, lds_bytes, bs, n, h, ch, 1024, 4, gm))) return r;
        c.ntiles = h.ntiles;
        c.tiles_per_stripe = h.tiles_per_stripe;
        c.tile_order = g_tune.stream_order;
        int grid = h.grid;
        int chunk = g_tune.stream_chunk;
        if (chunk < 0) chunk = h.lds <= 8192 ? (outputs_consecutive(c, bs) ? 2 : 1) : 0;
        if (chunk > 0) {  // contiguous ranges of `chunk` tiles, one per workgroup
            const uint64_t per = static_cast<uint64_t>(chunk);
            grid = static_cast<int>(std::min<uint64_t>((h.ntiles + per - 1) / per, 1u << 30));
            c.tile_order = 1;
        }
        return launch_stream(c, width, ch, g_tune.stream_pf != 0, nib, dim3(grid), dim3(h.threads), h.lds, st);
    });
}

template <int W>
int launch_ptrs_w(const ApplyArgs& a, dim3 grid, dim3 block, size_t lds, hipStream_t st)
{
    switch ((a.ncols + 3) / 4) {
    case 1: hipLaunchKernelGGL((gf16_ptrs_stream_kernel<W, 1>), grid, block, lds, st, a); break;
    case 2: hipLaunchKernelGGL((gf16_ptrs_stream_kernel<W, 2>), grid, block, lds, st, a); break;
    case 3: hipLaunchKernelGGL((gf16_ptrs_stream_kernel<W, 3>), grid, block, lds, st, a); break;
    case 4: hipLaunchKernelGGL((gf16_ptrs_stream_kernel<W, 4>), grid, block, lds, st, a); break;
    default: hipLaunchKernelGGL((gf16_ptrs_stream_kernel<W, 5>), grid, block, lds, st, a); break;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ptrs_stream(const ApplyArgs& a, int width, dim3 grid, dim3 block, size_t lds, hipStream_t st)
{
    if (width == 2) return launch_ptrs_w<2>(a, grid, block, lds, st);
    if (width == 4) return launch_ptrs_w<4>(a, grid, block, lds, st);
    return launch_ptrs_w<8>(a, grid, block, lds, st);
}

// The bitsliced form (host/bitslice.hpp, hip/ecamd_jit.hip) of output rows row0 .. row0+nrows-1
// (5..8 of them) over ALL K <= 32 inputs -- whatever column chunks and row widths the LDS-table
// passes use -- on the whole 16 KiB tiles of every fragment; returns the bytes it covered (0: not
// taken -- shape, knob, or the kernel is still compiling); the LDS-table passes of those rows then
// run on the rest of each fragment only.
// Copy-through (copy_off non-null: the framed encode / decode-join of map_apply_copy): input j is
// also stored at copy_base + s*copy_stride + copy_off[j] (< 0: not copied) as it is loaded, and
// when base.limited (objects shorter than the k payloads) only the whole tiles below base.min_len
// are taken -- the LDS-table passes run the rest byte-exactly.
// One-wave 4 KiB tiles for a bitsliced row group of `nrows` outputs (knobs bs_wave, bs_wave_min_rows,
// bs_wave_copy); `narrow`: the group takes the bitsliced kernel below bitslice_min_rows for it.
// Realigned copy-through inputs (knob bs_realign): the byte shift of each input's offset, and the
// buffer size the realigned kernel needs -- each input's last window ends at in_off + cover and the
// aligned chunk under it at the next 16-byte boundary, which stays in the object's last 16-byte
// granule (objects are 16-byte aligned).  No shift: `shifts` empty and the records unchanged.
uint32_t realign_records(const ApplyArgs& a, int K, int64_t cover, bool copy, std::vector<int>& shifts)
{
    shifts.clear();
    if (!copy || !g_tune.bs_realign) return a.in_records;
    bool any = false;
    int64_t end = 0;
    for (int j = 0; j < K; j++) {
        shifts.push_back(a.in_off32[j] & 15);
        any = any || (a.in_off32[j] & 15);
        end = std::max<int64_t>(end, (static_cast<int64_t>(a.in_off32[j]) + cover + 15) & ~int64_t(15));
    }
    if (!any) {
        shifts.clear();
        return a.in_records;
    }
    // exactly `end`: the caller's records (max in_off + bs) may stop inside the last aligned chunk
    // when bs is the covered range itself, and the buffer unit zeroes every dword past the records
    return static_cast<uint32_t>(end);
}

bool bs_wave_tiles(int nrows, int K, bool copy, bool* narrow, bool unaligned = false)
{
    const bool ok = !copy || g_tune.bs_wave_copy == 1 || (g_tune.bs_wave_copy == 2 && unaligned && g_tune.bs_realign);
    // 1-2 outputs (single-destination reconstruct, 1-2 lost): bitsliced when the map has at least
    // bs_narrow_min_k inputs (the LDS tables are K x 2 KiB there, and small at C2's k = 4)
    const bool few = nrows <= 2 && g_tune.bs_narrow_min_k > 0 && K >= g_tune.bs_narrow_min_k;
    const bool n = ok && g_tune.bs_wave >= 1 && (nrows >= g_tune.bs_wave_min_rows || few) && nrows <= 4;
    if (narrow) *narrow = n;
    return ok && (n || g_tune.bs_wave == 2);
}

// The one-wave form's occupancy for an R-output map (BsOcc, host/bitslice.hpp): knobs bs_wave_wmin /
// bs_wave_wmax (0: the policy below) and bs_wave_barrier (< 0: the policy).
BsOcc wave_occ(int R, bool copy)
{
    // 2 waves per SIMD: the register budget the dense 3-4-output decode networks need without
    // spilling, and an occupancy cap (descriptor VGPRs padded to 176) -- which is also the rate's
    // optimum: more resident waves run SLOWER (C3 encode 0.745 at 2 per SIMD, 0.717 at 3, 0.711 at 4,
    // 0.68 at 1; profiles/r05_ab_occ.log, r05_ab_occ2.log), and the resident workgroups per CU are
    // then trimmed further (bs_wave_per_cu).  Plain maps close each input's network with a scheduling
    // barrier (the next input's loads are not hoisted into it: fewer live registers, and 0.5-1%
    // faster at the same occupancy, r05_ab_occ2.log w22b); copy-through forms order their loads and
    // stores themselves (bs_prefetch).
    BsOcc o;
    o.wmin = 2;
    o.wmax = 2;
    o.barrier = !copy;
    if (g_tune.bs_wave_wmin > 0) o.wmin = g_tune.bs_wave_wmin;
    if (g_tune.bs_wave_wmax > 0) o.wmax = g_tune.bs_wave_wmax;
    if (g_tune.bs_wave_barrier >= 0) o.barrier = g_tune.bs_wave_barrier != 0;
    o.wmax = std::max(o.wmax, o.wmin);
    return o;
}

// Dynamic LDS per workgroup that caps the resident workgroups of a launch at n per CU (0: none).  The
// streaming kernels are HBM-pattern bound, and their rate peaks at a concurrency below what their
// registers allow: C3's one-wave bitsliced kernel runs 0.75 of 8 TB/s at 8 one-wave workgroups per
// CU, 0.81 at 7, 0.70 at 6 (tools/bs_wave_ab.py c3cap2, profiles/r05_ab_cap2.log).
size_t per_cu_lds(int n) { return n > 0 ? (kLdsBytes / static_cast<size_t>(n)) & ~size_t(511) : 0; }

// The dynamic LDS a launch of the module kernel fn adds so that its workgroup's LDS (static + dynamic)
// is per_cu_lds(n): 0 when n is 0 or the static share is already that large.
unsigned cap_lds(hipFunction_t fn, int n)
{
    const size_t want = per_cu_lds(n);
    if (!want || !fn) return 0;
    int stat = 0;
    if (hipFuncGetAttribute(&stat, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, fn) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return want > static_cast<size_t>(stat) ? static_cast<unsigned>(want - static_cast<size_t>(stat)) : 0u;
}

// Whether a row group of nrows outputs over K inputs takes the bitsliced kernel under the current
// knobs, and in which form (launch_bitslice; ecamd_bitslice_prebuild and ecamd_rs_kernel_form ask
// the same question without launching).
struct BsForm {
    bool wave = false;  // one-wave 4 KiB tiles (else 4-wave 16 KiB tiles)
    int depth = 0;      // LDS ring depth (0: register loads)
    int prefetch = 0;   // BitsliceStyle::prefetch (copy-through forms)
    BsOcc occ;          // one-wave forms: occupancy (knobs bs_wave_wmin / bs_wave_wmax / bs_wave_barrier)
    int opts = 0;       // plain one-wave register form: kBsOpt* bits (knob bs_store_through, ecamd_bitslice_timeline)
};
// ecamd_bitslice_timeline's buffer (a development hook, measurement only): while set, the plain one-wave
// form runs its timeline form -- in every thread of the process, so the hook is for a tool that launches
// from one thread.  The two words are not set together: bs_form may still see the old count, and the
// launcher reads both again and hands the kernel a null buffer with a count of 0 whenever they disagree.
std::atomic<uint32_t*> g_timeline{nullptr};
std::atomic<uint32_t> g_timeline_records{0};
bool bs_form(int nrows, int K, bool copy, bool unaligned, BsForm& f)
{
    if (!g_tune.bitslice || nrows <= 0 || nrows > kBsMaxR || K <= 0 || K > kBsMaxK) return false;
    if (copy && bitslice_depth(g_tune.bitslice_depth, K) != 0) return false;  // ring form: no copy-through
    // one-wave 4 KiB tiles (knob bs_wave): 3-4-output maps (C3 encode and decodes) run best in the
    // finest dispatcher-balanced units the 4-chunk transpose allows -- interleaved output slots
    // ({0,5,10,13}) above all; 5-8-output maps keep the 4-wave 16 KiB tiles
    bool narrow = false;
    f.wave = bs_wave_tiles(nrows, K, copy, &narrow, unaligned);
    if (nrows < g_tune.bitslice_min_rows && !narrow) return false;
    // LDS ring (depth 2 / 4) or register loads: bs_wave_depth for one-wave plain maps, bitslice_depth
    // for 16 KiB tiles; copy-through maps always load into registers
    // (one-wave copy-through maps: an LDS ring only with knob bs_copy_ring, a development A/B)
    f.depth = copy ? (f.wave ? static_cast<int>(g_tune.bs_copy_ring) : 0)
                   : static_cast<int>(f.wave ? g_tune.bs_wave_depth : g_tune.bitslice_depth);
    f.prefetch = f.depth ? 0
                 : !copy ? (f.wave ? static_cast<int>(g_tune.bs_plain_prefetch) : 0)
                         : f.wave ? static_cast<int>(g_tune.bs_prefetch) : static_cast<int>(g_tune.bs_late_copy);
    f.occ = wave_occ(nrows, copy);
    f.opts = 0;
    if (f.wave && !copy && f.depth == 0) {
        const int through = static_cast<int>(g_tune.bs_store_through);
        f.opts = ((through < 0 ? nrows >= 2 && nrows <= 4 : through > 0) ? kBsOptStoreThrough : 0) |
                 (g_timeline_records.load(std::memory_order_relaxed) ? kBsOptTimeline : 0);
    }
    if (!f.wave) {  // multi-wave form: its workgroup size (plain register form only; bs_tile_threads)
        f.occ = BsOcc{};
        const int t = static_cast<int>(g_tune.bs_tile_threads);
        if (!copy && f.depth == 0 && (t == 128 || t == 512)) f.occ.threads = t;
    }
    return true;
}

// Lanes per workgroup and bytes of each fragment per tile of a form.
int bs_threads(const BsForm& f) { return f.wave ? 64 : f.occ.threads ? f.occ.threads : 256; }

// chk (ecamd_rs_check): the map is a syndrome matrix [A | I] whose last nrows inputs are the stored
// fragments under test; the check form of the kernel writes no fragment (out_off unused) and ORs
// bit chk->bits[r] into chk->status[stripe] for every row r whose syndrome is not zero.
// With `suspects` (ecamd_rs_locate) the kernel is the locate form: a wave that sees a non-zero syndrome
// also ANDs the mask of the candidates that explain it into suspects[stripe]; frag_bits[i] is the
// fragment index of the map's input i (the K inputs, then the checked rows).
struct BsCheck {
    uint32_t* status;
    const uint8_t* bits;
    uint32_t* suspects = nullptr;
    const uint8_t* frag_bits = nullptr;
};
std::atomic<long long> g_check_fused{0};  // check-form launches enqueued by this process
std::atomic<long long> g_locate_fused{0};  // locate-form launches

int64_t launch_bitslice(const ecamd_map* map, int row0, int nrows, const ApplyArgs& base,
                        const int64_t* in_off, const int64_t* out_off, int64_t bs, int nstripes,
                        hipStream_t st, int* rc, const int64_t* copy_off = nullptr, const BsCheck* chk = nullptr)
{
    *rc = 0;
    const int mode = g_tune.bitslice;
    const int K = map->K;
    if (!copy_off && (base.copy_records || base.limited)) return 0;
    bool unaligned = false;
    for (int j = 0; j < K && j < kBsMaxK; j++) unaligned = unaligned || (in_off[j] & 15);
    BsForm form;
    if (!bs_form(nrows, K, copy_off != nullptr, unaligned, form)) return 0;
    ApplyArgs a = base;
    a.ncols = K;
    a.nrows = chk ? 0 : nrows;
    for (int j = 0; j < K; j++) a.in_off[j] = in_off[j];
    for (int r = 0; r < a.nrows; r++) a.out_off[r] = out_off[row0 + r];
    const bool wave = form.wave;
    const int threads = bs_threads(form);
    const int64_t tile = static_cast<int64_t>(threads) * 64;  // kBsTileWave / kBsTile at 64 / 256 lanes
    if (bs < tile) return 0;
    const int64_t cover = (base.limited ? std::min<int64_t>(bs, base.min_len) : bs) / tile * tile;
    if (cover < tile) return 0;
    if (!stream_offsets(a, bs)) return 0;
    if (copy_off) {
        for (int j = 0; j < K; j++) a.copy_off[j] = copy_off[j];
        if (!stream_copy_offsets(a, bs)) return 0;
    }
    std::vector<int> sub(static_cast<size_t>(nrows) * K);
    for (int r = 0; r < nrows; r++)
        for (int j = 0; j < K; j++)
            sub[static_cast<size_t>(r) * K + j] = map->coeff[static_cast<size_t>(row0 + r) * K + j];
    std::shared_ptr<void> hold;  // the kernel's module stays loaded until the launch is enqueued
    std::vector<int> shifts;
    const uint32_t in_records = realign_records(a, K, cover, copy_off != nullptr, shifts);
    hipFunction_t fn = bitslice_function(map->device, sub, nrows, K, form.depth, mode == 2, hold, copy_off != nullptr,
                                         0, wave, &shifts, form.prefetch, nullptr, &form.occ, chk != nullptr,
                                         chk && chk->suspects, chk ? 0 : form.opts);
    if (!fn) return 0;
    BsArgs b{};
    b.in_base = a.in_base;
    b.out_base = a.out_base;
    b.in_stride = a.in_stride;
    b.out_stride = a.out_stride;
    b.stripe_list = a.stripe_list;
    b.in_records = in_records;
    b.out_records = a.out_records;
    b.tiles_per_stripe = static_cast<uint32_t>(cover / tile);
    b.ntiles = b.tiles_per_stripe * static_cast<uint32_t>(nstripes);
    for (int j = 0; j < K; j++) b.in_off[j] = a.in_off32[j];
    for (int r = 0; r < a.nrows; r++) b.out_off[r] = a.out_off32[r];
    if (chk) {
        b.status = chk->status;
        for (int r = 0; r < nrows; r++) b.status_bit[r] = chk->bits[row0 + r];
        if (chk->suspects) {
            b.suspects = chk->suspects;
            for (int j = 0; j < K; j++) b.frag_bit[j] = chk->frag_bits[j];
        }
    }
    if (copy_off) {  // offsets as idx * step (the kernel keeps 8 scalar registers, not 32)
        int64_t step = 0;
        for (int j = 0; j < K; j++)
            if (copy_off[j] > 0) step = std::gcd(step, copy_off[j]);
        if (step == 0) step = 1;
        for (int j = 0; j < K; j++) {
            if (copy_off[j] < 0) {
                b.copy_idx[j] = 0xff;
                continue;
            }
            const int64_t idx = copy_off[j] / step;
            if (idx > 254) return 0;
            b.copy_idx[j] = static_cast<uint8_t>(idx);
        }
        b.copy_base = a.copy_base;
        b.copy_stride = a.copy_stride;
        b.copy_records = a.copy_records;
        b.copy_step = static_cast<uint32_t>(step);
    }
    // 2 workgroups of 4 waves per CU: the network's ~240 VGPRs allow 2 waves per SIMD
    // one 4-wave workgroup per wave per SIMD the kernel is built for (2 for 5..8 outputs)
    // (one-wave workgroups: 4 per such slot, so a launch keeps its bytes)
    const int64_t slots = static_cast<int64_t>(cu_count(map->device)) * bitslice_waves_per_simd(nrows) * 4 * 64 / threads;
    // long passes as several launches (bs_tiles_per_slot; as launch_stream_pass)
    const uint64_t limit = static_cast<uint64_t>(std::max(0, static_cast<int>(g_tune.bs_tiles_per_slot)));
    int per = nstripes;
    if (limit && b.ntiles > limit * slots) {
        const uint64_t launches = (b.ntiles + limit * slots - 1) / (limit * slots);
        per = static_cast<int>((static_cast<uint64_t>(nstripes) + launches - 1) / launches);
    }
    for (int s0 = 0; s0 < nstripes && *rc == 0; s0 += per) {
        BsArgs c = b;
        const int n = std::min(per, nstripes - s0);
        if (b.stripe_list) {
            c.stripe_list = b.stripe_list + s0;
        } else {
            c.in_base = b.in_base + s0 * b.in_stride;
            c.out_base = b.out_base + s0 * b.out_stride;
            if (c.copy_records) c.copy_base = b.copy_base + s0 * b.copy_stride;
            if (chk) c.status = b.status + s0;  // the kernel indexes it by the launch's own stripe number
            if (chk && b.suspects) c.suspects = b.suspects + s0;
        }
        c.ntiles = b.tiles_per_stripe * static_cast<uint32_t>(n);
        // bs_grid 1: one workgroup per tile (the dispatcher balances the tiles); 0: the resident slots
        const int64_t grid = g_tune.bs_grid ? static_cast<int64_t>(c.ntiles) : std::min<int64_t>(c.ntiles, slots);
        // resident workgroups per CU: one-wave plain maps bs_wave_per_cu; copy-through maps bs_copy_per_cu
        // when every input is read aligned (C3 objects, decode-joins), bs_copy_realign_per_cu when inputs
        // are realigned in registers (Swift's segments); 16 KiB tiles bs_tile_per_cu
        // (the check form reads its K fragments, checked ones included, and writes none: knob check_per_cu)
        const int wg_cap = !wave ? static_cast<int>(g_tune.bs_tile_per_cu)
                        : chk ? (g_tune.check_per_cu >= 0 ? static_cast<int>(g_tune.check_per_cu) : K >= 20 ? 0 : 7)
                        : !copy_off ? (g_tune.bs_wave_per_cu >= 0 ? static_cast<int>(g_tune.bs_wave_per_cu)
                                                                   : K + nrows >= 20 ? 0 : 7)
                        : shifts.empty() ? static_cast<int>(g_tune.bs_copy_per_cu)
                                         : static_cast<int>(g_tune.bs_copy_realign_per_cu);
        const unsigned lds = cap_lds(fn, wg_cap);
        if (!chk && (form.opts & kBsOptTimeline)) {  // (only the timeline form's kernel reads these)
            // tile t of the pass: launches after the first continue the record numbering
            const uint32_t first = b.tiles_per_stripe * static_cast<uint32_t>(s0);
            const uint32_t total = g_timeline_records.load(std::memory_order_relaxed);
            uint32_t* buf = g_timeline.load(std::memory_order_relaxed);
            c.timeline = buf && total > first ? buf + static_cast<size_t>(first) * 8 : nullptr;
            c.timeline_records = c.timeline ? total - first : 0;
        }
        *rc = bitslice_launch(fn, c, static_cast<int>(grid), st, hold, threads, lds);
        if (chk && *rc == 0) (chk->suspects ? g_locate_fused : g_check_fused).fetch_add(1, std::memory_order_relaxed);
    }
    return *rc ? 0 : cover;
}

// Rows [row0, row0 + nrows) of the R x K matrix A as the syndrome matrix [A | I] over its K inputs
// followed by those rows' own fragments: the one place the run time's request (check_fused) and the
// shipped object's key (check_fused_prebuild) come from.
std::vector<int> syndrome_rows(const std::vector<int>& A, int K, int row0, int nrows)
{
    const int W = K + nrows;
    std::vector<int> syn(static_cast<size_t>(nrows) * W, 0);
    for (int r = 0; r < nrows; r++) {
        for (int j = 0; j < K; j++) syn[static_cast<size_t>(r) * W + j] = A[static_cast<size_t>(row0 + r) * K + j];
        syn[static_cast<size_t>(r) * W + K + r] = 1;
    }
    return syn;
}

}  // namespace

namespace ecamd {

int64_t check_fused(int dev, const std::vector<int>& A, int K, int row0, int nrows, const uint8_t* base,
                    int64_t stripe_stride, const int64_t* in_off, const int64_t* chk_off, const uint8_t* bits,
                    uint32_t* d_status, uint32_t* d_suspects, const uint8_t* in_bits, int64_t blocksize, int nstripes,
                    void* stream)
{
    if (nrows > kBsMaxR || K + nrows > kBsMaxK) return 0;
    ecamd_map syn;
    syn.device = dev;
    syn.R = nrows;
    syn.K = K + nrows;
    syn.coeff = syndrome_rows(A, K, row0, nrows);
    std::vector<int64_t> off(in_off, in_off + K);
    off.insert(off.end(), chk_off + row0, chk_off + row0 + nrows);
    std::vector<uint8_t> frag_bits(in_bits, in_bits + K);  // of the map's inputs: the K inputs, then the checked rows
    frag_bits.insert(frag_bits.end(), bits + row0, bits + row0 + nrows);
    ApplyArgs a{};
    a.in_base = base;
    a.in_stride = stripe_stride;
    const BsCheck chk{d_status, bits + row0, d_suspects, frag_bits.data()};
    int rc = 0;
    const int64_t cover = launch_bitslice(&syn, 0, nrows, a, off.data(), nullptr, blocksize, nstripes,
                                          static_cast<hipStream_t>(stream), &rc, nullptr, &chk);
    return rc ? rc : cover;
}

int check_fused_prebuild(const std::vector<int>& A, int K, int row0, int nrows, bool locate, const char* arch,
                         const char* dir)
{
    BsForm f;
    if (nrows > kBsMaxR || K + nrows > kBsMaxK || !bs_form(nrows, K + nrows, false, false, f)) return 0;
    return bitslice_prebuild(syndrome_rows(A, K, row0, nrows), nrows, K + nrows, f.depth, false, 0, f.wave, nullptr,
                             f.prefetch, f.occ, arch, dir, true, locate);
}

}  // namespace ecamd

namespace {

template <bool PTRS>
int launch_gf16(const ecamd_map* map, ApplyArgs base_args, const int64_t* in_off,
                const int64_t* out_off, int64_t bs_all, int nstripes, hipStream_t st)
{
    // bytes of each fragment the bitsliced kernel covered, per group of 8 output rows (the LDS-table
    // row widths 2 / 4 / 8 divide 8, so a pass lies in one group)
    std::vector<int64_t> bs_done(static_cast<size_t>((map->R + 7) / 8), 0);
    // launches small enough for gf16_small_kernel skip the bitsliced one: a per-call 64 KiB object
    // (6.5 KiB fragments) paid a 12 us one-tile bitsliced launch and a 12 us small launch for the rest.
    // Only when small_launch() takes EVERY pass of the row group: a pass it declines (permuted survivors,
    // unaligned bases) would otherwise get the stream kernel over the whole fragment
    auto group_small = [&](int g) {
        if ((bs_all + 15) / 16 * nstripes > g_tune.small_chunks) return false;
        bool any = false;
        for (const auto& p : map->passes) {
            if (p.row0 / 8 != g) continue;
            ApplyArgs a = base_args;
            a.ncols = p.ncols;
            a.nrows = std::min(p.width, map->R - p.row0);
            for (int j = 0; j < p.ncols; j++) a.in_off[j] = in_off[p.col0 + j];
            for (int r = 0; r < a.nrows; r++) a.out_off[r] = out_off[p.row0 + r];
            if (!small_launch(a, bs_all, nstripes)) return false;
            any = true;
        }
        return any;
    };
    if constexpr (!PTRS) {
        for (int g = 0; g * 8 < map->R; g++) {
            if (group_small(g)) continue;
            int brc = 0;
            bs_done[static_cast<size_t>(g)] = launch_bitslice(map, g * 8, std::min(8, map->R - g * 8), base_args, in_off, out_off,
                                         bs_all, nstripes, st, &brc);
            if (brc) return brc;
        }
    }
    for (const auto& p : map->passes) {
        ApplyArgs a = base_args;
        int64_t bs = bs_all;
        const int64_t done = bs_done[static_cast<size_t>(p.row0 / 8)];
        if (done == bs_all) continue;
        a.tables = map->d_tables + p.offset;
        a.bs = bs;
        a.ncols = p.ncols;
        a.nrows = std::min(p.width, map->R - p.row0);
        a.accumulate = p.col0 > 0;
        for (int j = 0; j < p.ncols; j++) a.in_off[j] = in_off[p.col0 + j];
        for (int r = 0; r < a.nrows; r++) a.out_off[r] = out_off[p.row0 + r];
        if constexpr (!PTRS) {
            if (done > 0) {  // the tail of every fragment through the LDS-table kernels
                for (int j = 0; j < p.ncols; j++) a.in_off[j] += done;
                for (int r = 0; r < a.nrows; r++) a.out_off[r] += done;
                bs -= done;
                a.bs = bs;
            }
        }
        if (!PTRS && small_launch(a, bs, nstripes)) {
            int rc = launch_small(a, p, bs, nstripes, map->d_tables, map->serial, st, nullptr,
                                  &p == &map->passes.back(), map->passes.size() == 1 && done == 0);
            if (rc) return rc;
            continue;
        }
        Geometry g;
        int rc = geometry(map->device, p.bytes, bs, nstripes, g, 1);
        if (rc) return rc;
        a.ntiles = g.ntiles;
        a.tiles_per_stripe = g.tiles_per_stripe;
        dim3 grid(g.grid), block(g.threads);
        if (!PTRS && g_tune.nt && g_tune.stream && p.ncols <= 4 * kStreamGroups &&
            stream_offsets(a, bs)) {
            const bool nib = g_tune.stream_nib == 1 || (g_tune.stream_nib == 2 && p.width == 8) ||
                             (g_tune.nib != 0);
            const int ch = (p.width <= 4 && !nib) ? g_tune.stream_ch : 1;
            if (nib) a.tables = map->d_tables + p.nib_offset;
            // 16 waves per CU (4 x 256 threads, or fewer, larger workgroups when the tables
            // allow fewer than 4): measured best for this kernel at C2 / C3 / C5
            rc = launch_stream_pass(a, map->device, nib ? p.nib_bytes : p.bytes, p.width, ch, nib, bs,
                                    nstripes, st);
            if (rc) return rc;
            continue;
        }
        if (a.stripe_list)  // only the stream kernel reads a stripe list
            return fail(ECAMD_EINVAL, "stripe list on a non-stream launch");
        if (PTRS && g_tune.nt && g_tune.stream && p.ncols <= 4 * kStreamGroups &&
            bs < (int64_t(1) << 31)) {
            rc = geometry(map->device, p.bytes, bs, nstripes, g, 1, 1024, 4);
            if (rc) return rc;
            a.ntiles = g.ntiles;
            a.tiles_per_stripe = g.tiles_per_stripe;
            rc = launch_ptrs_stream(a, p.width, dim3(g.grid), dim3(g.threads), g.lds, st);
            if (rc) return rc;
            continue;
        }
        if (g_tune.nib) {
            a.tables = map->d_tables + p.nib_offset;
            rc = geometry(map->device, p.nib_bytes, bs, nstripes, g);
            if (rc) return rc;
            if (g.threads > 512) {  // the nibble kernels are built for <= 512 threads
                rc = geometry(map->device, p.nib_bytes, bs, nstripes, g, 1, 512);
                if (rc) return rc;
            }
            a.ntiles = g.ntiles;
            a.tiles_per_stripe = g.tiles_per_stripe;
            grid = dim3(g.grid);
            block = dim3(g.threads);
            switch (p.width) {
            case 2: hipLaunchKernelGGL((gf16_apply_kernel<2, PTRS, true, true>), grid, block, g.lds, st, a); break;
            case 4: hipLaunchKernelGGL((gf16_apply_kernel<4, PTRS, true, true>), grid, block, g.lds, st, a); break;
            default: hipLaunchKernelGGL((gf16_apply_kernel<8, PTRS, true, true>), grid, block, g.lds, st, a); break;
            }
            HIP_TRY(hipGetLastError());
            continue;
        }
        const bool nt = g_tune.nt != 0;
        switch (p.width * 2 + (nt ? 1 : 0)) {
        case 4: hipLaunchKernelGGL((gf16_apply_kernel<2, PTRS, false, false>), grid, block, g.lds, st, a); break;
        case 5: hipLaunchKernelGGL((gf16_apply_kernel<2, PTRS, true, false>), grid, block, g.lds, st, a); break;
        case 8: hipLaunchKernelGGL((gf16_apply_kernel<4, PTRS, false, false>), grid, block, g.lds, st, a); break;
        case 9: hipLaunchKernelGGL((gf16_apply_kernel<4, PTRS, true, false>), grid, block, g.lds, st, a); break;
        case 16: hipLaunchKernelGGL((gf16_apply_kernel<8, PTRS, false, false>), grid, block, g.lds, st, a); break;
        default: hipLaunchKernelGGL((gf16_apply_kernel<8, PTRS, true, false>), grid, block, g.lds, st, a); break;
        }
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

constexpr int64_t kXorNarrowMin = 256 << 10;  // fragment bytes from which flat XOR takes 1 KiB tiles
std::atomic<long long> g_xor_stream_launches{0};  // xor_stream_kernel launches enqueued by this process

// copy_off (framed flat-XOR encode): input j is also stored at base_args.copy_base + s*copy_stride +
// copy_off[j] by the first row group's launches -- whole stream-kernel tiles only: ECAMD_EINVAL, with
// nothing launched, unless bs is a multiple of the tile and every offset fits the stream kernel.
template <bool PTRS>
int launch_xor(const uint32_t* masks, int R, int K, ApplyArgs base_args, const int64_t* in_off,
               const int64_t* out_off, int64_t bs, int nstripes, hipStream_t st,
               const int64_t* copy_off = nullptr)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (copy_off) {  // check the whole plan before the first launch
        if (PTRS || K > 32 || !g_tune.stream || bs % 4096) return ECAMD_EINVAL;
        ApplyArgs t = base_args;
        t.ncols = K;
        t.nrows = std::min(kMaxRows, R);
        for (int j = 0; j < K; j++) {
            t.in_off[j] = in_off[j];
            t.copy_off[j] = copy_off[j];
        }
        for (int r = 0; r < t.nrows; r++) t.out_off[r] = out_off[r];
        if (!stream_offsets(t, bs) || !stream_copy_offsets(t, bs)) return ECAMD_EINVAL;
        for (int row0 = kMaxRows; row0 < R; row0 += kMaxRows) {
            ApplyArgs u = t;
            u.nrows = std::min(kMaxRows, R - row0);
            for (int r = 0; r < u.nrows; r++) u.out_off[r] = out_off[row0 + r];
            if (!stream_offsets(u, bs)) return ECAMD_EINVAL;
        }
    }
    for (int row0 = 0; row0 < R; row0 += kMaxRows) {
        for (int col0 = 0; col0 < K; col0 += 32) {
            ApplyArgs a = base_args;
            a.bs = bs;
            a.ncols = std::min(32, K - col0);
            a.nrows = std::min(kMaxRows, R - row0);
            a.accumulate = col0 > 0;
            for (int j = 0; j < a.ncols; j++) a.in_off[j] = in_off[col0 + j];
            for (int r = 0; r < a.nrows; r++) {
                a.out_off[r] = out_off[row0 + r];
                a.masks[r] = col0 < 32 ? (masks[row0 + r] >> col0) : 0u;
            }
            if (!PTRS && !copy_off && small_launch(a, bs, nstripes)) {
                int rc = launch_xor_small(a, bs, nstripes, st, row0 + kMaxRows >= R && col0 + 32 >= K, nullptr,
                                          R <= kMaxRows && K <= 32);
                if (rc) return rc;
                continue;
            }
            Geometry g;
            const bool use_stream = !PTRS && g_tune.stream && stream_offsets(a, bs);
            const bool copy = copy_off && row0 == 0;  // the first row group copies the inputs through
            if (copy) {
                for (int j = 0; j < a.ncols; j++) a.copy_off[j] = copy_off[col0 + j];
                if (!stream_copy_offsets(a, bs)) return fail(ECAMD_EINVAL, "xor copy-through offsets");
            } else {
                a.copy_records = 0;
            }
            const int xt = g_tune.xor_threads ? g_tune.xor_threads
                                               : (a.ncols > 4 && bs >= kXorNarrowMin ? 64 : 256);
            const bool narrow = use_stream && (xt == 64 || xt == 128);  // only the stream kernel
            int rc = geometry(dev, 0, bs, nstripes, g, 1, narrow ? xt : 1024);
            if (rc) return rc;
            a.ntiles = g.ntiles;
            a.tiles_per_stripe = g.tiles_per_stripe;
            if (use_stream) {
                // geometry: 256 threads, one workgroup per 4 KiB tile (xor_grid; the dispatcher
                // hands each freed slot the next tile: (10,6,4) encode 0.753 -> 0.790 of 8 TB/s,
                // (3,3,3) 0.717 -> 0.743, profiles/r03_xor_grid.log); long passes as several
                // launches of xor_tiles_per_slot tiles per slot (as launch_stream_pass), slots =
                // xor_wgs per CU -- by default 3 for passes of more than 4 inputs into 3+ outputs,
                // else 2 (tools/xor_geom_sweep.py, profiles/r03_xor_geom.log)
                const int wgs = g_tune.xor_wgs > 0 ? g_tune.xor_wgs : (a.ncols > 4 && a.nrows >= 3 ? 3 : 2);
                const int64_t slots = static_cast<int64_t>(cu_count(dev)) * wgs;
                // narrower tiles: the same bytes per launch (tiles per slot scaled by 256 / threads)
                const int knob = g_tune.xor_tiles_per_slot * (256 / g.threads);
                rc = for_each_launch(a, nstripes, g.tiles_per_stripe, static_cast<uint64_t>(slots),
                                     static_cast<uint64_t>(std::max(knob, 0)), [&](ApplyArgs& c, int n) {
                    c.ntiles = g.tiles_per_stripe * static_cast<uint32_t>(n);
                    const dim3 grid(static_cast<int>(std::max<int64_t>(
                        1, g_tune.xor_grid ? static_cast<int64_t>(c.ntiles) : std::min<int64_t>(c.ntiles, slots)))),
                        block(g.threads);
                    // resident workgroups per CU: knob xor_per_cu (< 0: 6 for 4 KiB tiles of more than 4
                    // inputs -- (10,6,4) at 64 KiB 0.754 -> 0.791, at 16 KiB 0.751 -> 0.758; one-wave tiles
                    // and small codes lose with any cap, tools/xor_threads_ab.py, profiles/r05_ab_xorcap.log)
                    const int xcap = g_tune.xor_per_cu >= 0 ? static_cast<int>(g_tune.xor_per_cu)
                                                            : (g.threads == 256 && c.ncols > 4 ? 6 : 0);
                    const size_t lds = per_cu_lds(xcap);
                    if (copy) {  // (for_each_launch advanced copy_base with the stripes)
                        switch ((c.ncols + 3) / 4) {
                        case 1: hipLaunchKernelGGL((xor_stream_kernel<1, true>), grid, block, lds, st, c); break;
                        case 2: hipLaunchKernelGGL((xor_stream_kernel<2, true>), grid, block, lds, st, c); break;
                        case 3: hipLaunchKernelGGL((xor_stream_kernel<3, true>), grid, block, lds, st, c); break;
                        case 4: hipLaunchKernelGGL((xor_stream_kernel<4, true>), grid, block, lds, st, c); break;
                        default: hipLaunchKernelGGL((xor_stream_kernel<8, true>), grid, block, lds, st, c); break;
                        }
                    } else {
                        switch ((c.ncols + 3) / 4) {
                        case 1: hipLaunchKernelGGL((xor_stream_kernel<1, false>), grid, block, lds, st, c); break;
                        case 2: hipLaunchKernelGGL((xor_stream_kernel<2, false>), grid, block, lds, st, c); break;
                        case 3: hipLaunchKernelGGL((xor_stream_kernel<3, false>), grid, block, lds, st, c); break;
                        case 4: hipLaunchKernelGGL((xor_stream_kernel<4, false>), grid, block, lds, st, c); break;
                        default: hipLaunchKernelGGL((xor_stream_kernel<8, false>), grid, block, lds, st, c); break;
                        }
                    }
                    g_xor_stream_launches.fetch_add(1, std::memory_order_relaxed);
                    HIP_TRY(hipGetLastError());
                    return 0;
                });
                if (rc) return rc;
            } else {
                if (a.stripe_list)  // only the stream kernel reads a stripe list
                    return fail(ECAMD_EINVAL, "stripe list on a non-stream xor launch");
                hipLaunchKernelGGL((xor_apply_kernel<8, PTRS>), dim3(g.grid), dim3(g.threads), 0, st,
                                   a);
            }
            HIP_TRY(hipGetLastError());
        }
    }
    return 0;
}

// ---- cached liberasurecode_rs_vand maps ------------------------------------------------

struct RsEntry {
    std::unique_ptr<ecamd_map, void (*)(ecamd_map*)> map{nullptr, ecamd_map_destroy};
    std::vector<int> inputs, outputs;
    // check maps only (kind 4): the pair table of check_map_pairs, made once on demand
    std::once_flag pairs_once;
    PairsTable pairs;
    int pairs_rc = 0;
    void* pairs_dev = nullptr;
    // and the correction table of check_map_correct, the same way
    std::once_flag correct_once;
    CorrectTable correct;
    int correct_rc = 0;
    void* correct_dev = nullptr;
    ~RsEntry()
    {
        if (pairs_dev) (void)hipFree(pairs_dev);
        if (correct_dev) (void)hipFree(correct_dev);
    }
};

// Bounded LRU of prepared maps keyed by (device, kind, k, m, rebuild, dest, erasures): a long-lived
// process that sees many distinct erasure patterns (k+m up to 256) keeps at most
// kCacheBytes of coefficient tables on each device.  Evicted entries stay alive while a launch
// still holds them (shared_ptr); their device tables are freed with the last reference.
constexpr size_t kCacheBytes = size_t(64) << 20;
struct CacheSlot {
    std::shared_ptr<RsEntry> entry;
    std::list<std::vector<int>>::iterator lru;
    size_t bytes;
};
std::mutex g_cache_mu;
std::map<std::vector<int>, CacheSlot> g_cache;
std::list<std::vector<int>> g_lru;  // most recent first
size_t g_cache_bytes = 0;

size_t map_bytes(const ecamd_map* mp)
{
    if (!mp || mp->passes.empty()) return 0;
    const auto& p = mp->passes.back();
    return std::max(p.offset + p.bytes, p.nib_offset + p.nib_bytes);
}

// caller holds g_cache_mu
void cache_insert(const std::vector<int>& key, std::shared_ptr<RsEntry>& e)
{
    auto it = g_cache.find(key);
    if (it != g_cache.end()) {  // another thread prepared it meanwhile
        e = it->second.entry;
        return;
    }
    g_lru.push_front(key);
    const size_t b = map_bytes(e->map.get()) + 256;
    g_cache.emplace(key, CacheSlot{e, g_lru.begin(), b});
    g_cache_bytes += b;
    while (g_cache_bytes > kCacheBytes && g_lru.size() > 1) {
        auto victim = g_cache.find(g_lru.back());
        g_cache_bytes -= victim->second.bytes;
        g_cache.erase(victim);
        g_lru.pop_back();
    }
}

int rs_entry(int kind, int k, int m, const int* missing, int rebuild, int dest,
             std::shared_ptr<RsEntry>& out)
{
    int dev = 0;
    int rc = ensure_device(&dev);
    if (rc) return rc;
    if (k <= 0 || m < 0 || k + m > 65536) return fail(ECAMD_EINVAL, "bad k=%d m=%d", k, m);
    std::vector<int> miss;
    if (missing)
        for (int i = 0; missing[i] > -1; i++) miss.push_back(missing[i]);
    std::vector<int> key = {dev, kind, k, m, rebuild, dest};
    key.insert(key.end(), miss.begin(), miss.end());
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        auto it = g_cache.find(key);
        if (it != g_cache.end()) {
            g_lru.splice(g_lru.begin(), g_lru, it->second.lru);
            out = it->second.entry;
            return 0;
        }
    }
    std::vector<int> G = rs_generator(k, m);
    if (G.empty()) return fail(ECAMD_EINVAL, "no generator for k=%d m=%d", k, m);
    FragmentMap fm;
    if (kind == 0)
        fm = rs_encode_map(G, k, m);
    else if (kind == 1) {
        if (rs_decode_map(G, k, m, miss, rebuild != 0, fm) != 0)
            return fail(ECAMD_EINVAL, "too many missing fragments (%zu > m=%d)", miss.size(), m);
    } else if (kind == 4) {  // ecamd_rs_check: every surviving fragment beyond the first k
        if (rs_check_map(G, k, m, miss, fm) != 0)
            return fail(ECAMD_EINVAL, "too many missing fragments (%zu > m=%d)", miss.size(), m);
    } else {
        if (rs_reconstruct_map(G, k, m, miss, dest, fm) != 0)
            return fail(ECAMD_EINVAL, "cannot reconstruct %d", dest);
    }
    auto e = std::make_shared<RsEntry>();
    e->inputs = fm.inputs;
    e->outputs = fm.outputs;
    if (!fm.outputs.empty() && !fm.inputs.empty()) {
        ecamd_map* mp = nullptr;
        rc = ecamd_map_create(fm.coeff.data(), static_cast<int>(fm.outputs.size()),
                              static_cast<int>(fm.inputs.size()), &mp);
        if (rc) return rc;
        e->map.reset(mp);
    }
    std::lock_guard<std::mutex> lk(g_cache_mu);
    cache_insert(key, e);
    out = e;
    return 0;
}

int rs_run(const RsEntry& e, void* base, int64_t stripe_stride, int64_t frag_stride, int64_t bs,
           int nstripes, void* stream)
{
    if (e.outputs.empty() || nstripes <= 0 || bs <= 0) return 0;
    if (e.inputs.empty()) {  // every input aliased away: the output is all zeros
        for (int s = 0; s < nstripes; s++)
            for (int o : e.outputs)
                HIP_TRY(hipMemsetAsync(static_cast<uint8_t*>(base) + s * stripe_stride +
                                           o * frag_stride, 0, bs,
                                       static_cast<hipStream_t>(stream)));
        return 0;
    }
    std::vector<int64_t> in_off, out_off;
    for (int i : e.inputs) in_off.push_back(i * frag_stride);
    for (int o : e.outputs) out_off.push_back(o * frag_stride);
    return ecamd_map_apply_strided(e.map.get(), base, stripe_stride, in_off.data(), base,
                                   stripe_stride, out_off.data(), bs, nstripes, stream);
}

}  // namespace

namespace ecamd {

int check_map(int k, int m, const int* missing, CheckMap& out)
{
    std::shared_ptr<RsEntry> e;
    const int rc = rs_entry(4, k, m, missing, 0, -1, e);
    if (rc) return rc;
    out.inputs = &e->inputs;
    out.checked = &e->outputs;
    out.map = e->map.get();
    out.coeff = e->map ? &e->map->coeff : nullptr;
    out.hold = e;
    return 0;
}

int check_map_pairs(const CheckMap& cm, PairsTable& out)
{
    out = PairsTable();
    auto* e = const_cast<RsEntry*>(static_cast<const RsEntry*>(cm.hold.get()));
    if (!e || !cm.coeff) return 0;
    std::call_once(e->pairs_once, [e, &cm] {
        const int K = static_cast<int>(e->inputs.size()), R = static_cast<int>(e->outputs.size());
        const PairPlan plan = rs_locate_pairs_plan(*cm.coeff, R, K);
        if (!plan.pairs || !plan.independent4) return;  // no table: d_pairs stays zero
        const GF16& gf = GF16::get();
        const int P = K + R, stride = 2 + R;
        auto frag = [&](int c) { return static_cast<uint32_t>(c < K ? e->inputs[c] : e->outputs[c - K]); };
        std::vector<uint32_t> tab;
        for (int c = 0; c < P; c++) {  // the single participants
            std::vector<int> col(static_cast<size_t>(R));
            int p = -1;
            uint32_t rows = 0;
            for (int r = 0; r < R; r++) {
                col[r] = c < K ? (*cm.coeff)[static_cast<size_t>(r) * K + c] : (r == c - K);
                if (col[r]) {
                    if (p < 0) p = r;
                    rows |= 1u << r;
                }
            }
            // (an all-zero column cannot be independent of the others)
            tab.push_back(frag(c) | 0xffu << 8 | static_cast<uint32_t>(std::max(p, 0)) << 16 | 0xffu << 24);
            tab.push_back(rows);
            for (int r = 0; r < R; r++) tab.push_back(p < 0 ? 0u : static_cast<uint32_t>(gf.mul(col[r], gf.inv(col[p]))));
        }
        int npairs = 0, i = 0;
        for (int a = 0; a < P; a++)
            for (int b = a + 1; b < P; b++, i++) {
                const int p = plan.pivot[static_cast<size_t>(i) * 2], q = plan.pivot[static_cast<size_t>(i) * 2 + 1];
                if (p < 0) continue;
                tab.push_back(frag(a) | frag(b) << 8 | static_cast<uint32_t>(p) << 16 | static_cast<uint32_t>(q) << 24);
                tab.push_back(0u);
                for (int r = 0; r < R; r++) {
                    const int* l = &plan.L[(static_cast<size_t>(i) * R + r) * 2];
                    tab.push_back(static_cast<uint32_t>(l[0]) | static_cast<uint32_t>(l[1]) << 16);
                }
                npairs++;
            }
        hipError_t err = hipMalloc(&e->pairs_dev, tab.size() * sizeof(uint32_t));
        if (err == hipSuccess) err = hipMemcpy(e->pairs_dev, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (err != hipSuccess) {
            e->pairs_rc = fail(ECAMD_EHIP, "pair table: %s", hipGetErrorString(err));
            return;
        }
        e->pairs.dev = static_cast<const uint32_t*>(e->pairs_dev);
        e->pairs.singles = P;
        e->pairs.pairs = npairs;
        e->pairs.stride = stride;
        e->pairs.exact = true;
    });
    if (e->pairs_rc) return fail(ECAMD_EHIP, "pair table upload failed");
    out = e->pairs;
    return 0;
}

int check_map_correct(const CheckMap& cm, CorrectTable& out)
{
    out = CorrectTable();
    auto* e = const_cast<RsEntry*>(static_cast<const RsEntry*>(cm.hold.get()));
    if (!e || !cm.coeff) return 0;  // nothing checked: nothing to correct
    std::call_once(e->correct_once, [e, &cm] {
        const int K = static_cast<int>(e->inputs.size()), R = static_cast<int>(e->outputs.size());
        const CorrectPlan plan = rs_correct_plan(*cm.coeff, R, K);
        const int P = K + R;
        if (P > 32 || static_cast<int>(plan.pivot.size()) != P) return;
        std::vector<uint32_t> tab(32, 0xffffffffu);
        for (int c = 0; c < P; c++) {
            const int f = c < K ? e->inputs[c] : e->outputs[c - K];
            if (f < 0 || f >= 32 || plan.pivot[c] < 0) continue;
            tab[static_cast<size_t>(f)] = static_cast<uint32_t>(c) | static_cast<uint32_t>(plan.pivot[c]) << 8 |
                                          static_cast<uint32_t>(plan.scale[c]) << 16;
        }
        for (int i = 0; i < plan.pairs; i++) {
            const int p = plan.pair_pivot[static_cast<size_t>(i) * 2], q = plan.pair_pivot[static_cast<size_t>(i) * 2 + 1];
            const int* w = &plan.minv[static_cast<size_t>(i) * 4];
            tab.push_back(p < 0 ? 0xffffu : static_cast<uint32_t>(p) | static_cast<uint32_t>(q) << 8);
            tab.push_back(static_cast<uint32_t>(w[0]) | static_cast<uint32_t>(w[1]) << 16);
            tab.push_back(static_cast<uint32_t>(w[2]) | static_cast<uint32_t>(w[3]) << 16);
        }
        // once per cached map, before anything of the call is enqueued: a few KiB, as the pair table
        hipError_t err = hipMalloc(&e->correct_dev, tab.size() * sizeof(uint32_t));
        if (err == hipSuccess) err = hipMemcpy(e->correct_dev, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (err != hipSuccess) {
            e->correct_rc = fail(ECAMD_EHIP, "correction table: %s", hipGetErrorString(err));
            return;
        }
        e->correct.dev = static_cast<const uint32_t*>(e->correct_dev);
        e->correct.pairs = plan.pairs > 0;
    });
    if (e->correct_rc) return fail(ECAMD_EHIP, "correction table upload failed");
    out = e->correct;
    return 0;
}

namespace {

// Copy-through launch of a cached rs map: input j of stripe s at in_base + s*in_stride +
// in_off[j] (map column order), output r at out_base + s*out_stride + out_off[r]; the first row
// group also stores input j at copy_base + s*copy_stride + copy_off[j] when copy_off[j] >= 0.
int map_apply_copy(const RsEntry& e, const uint8_t* in_base, int64_t in_stride,
                   const std::vector<int64_t>& in_off, uint8_t* out_base, int64_t out_stride,
                   const std::vector<int64_t>& out_off, uint8_t* copy_base, int64_t copy_stride,
                   const std::vector<int64_t>& copy_off, int64_t bs, int nstripes, void* stream,
                   const std::vector<int64_t>* in_len = nullptr,
                   const std::vector<int64_t>* out_len = nullptr,
                   const std::vector<int64_t>* copy_len = nullptr)
{
    const ecamd_map* map = e.map.get();
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto len_of = [&](const std::vector<int64_t>* v, int i) { return v ? (*v)[static_cast<size_t>(i)] : bs; };
    // Row groups of 5..8 outputs first take the bitsliced kernel over the whole 16 KiB tiles that
    // every input / copy / output fully holds (the first group copying the inputs through); the
    // LDS-table passes of those rows then run on the rest of each fragment only.
    std::vector<int64_t> bs_done(static_cast<size_t>((map->R + 7) / 8), 0);
    // knob frame_tail_fork: the LDS-table passes over each fragment's rest run on a side stream
    // beside the bitsliced launch (disjoint bytes) when that rest is 1-4 KiB -- one LDS-table launch
    // -- or, at 2, any rest; `pst` is the stream the passes go to
    hipStream_t pst = st;
    struct Joiner {  // error paths: the caller's stream still ends up after the side stream's work
        int dev;
        void* stream;
        bool on = false;
        ~Joiner()
        {
            if (on) (void)side_join(dev, stream);
        }
    } joiner{map->device, stream};
    {
        ApplyArgs b{};
        b.in_base = in_base;
        b.in_stride = in_stride;
        b.out_base = out_base;
        b.out_stride = out_stride;
        b.copy_base = copy_base;
        b.copy_stride = copy_stride;
        b.min_len = bs;
        for (int j = 0; j < map->K; j++) {
            b.min_len = std::min(b.min_len, len_of(in_len, j));
            if (copy_off[static_cast<size_t>(j)] >= 0) b.min_len = std::min(b.min_len, len_of(copy_len, j));
        }
        for (int r = 0; r < map->R; r++) b.min_len = std::min(b.min_len, len_of(out_len, r));
        b.limited = b.min_len < bs ? 1 : 0;
        // The bitsliced kernel covers whole 16 KiB tiles only; the rest of each fragment must then
        // run on the stream kernel (the pointer-free LDS-table kernels cannot start at an offset).
        // A row group whose passes cannot all take it (more than 20 inputs per pass, offsets past
        // 2 GiB) skips the bitsliced kernel instead of failing after writing part of the output.
        bool unaligned = false;
        for (int64_t o : in_off) unaligned = unaligned || (o & 15);
        auto cover_of = [&](int g) {  // bytes the group's bitsliced launch would cover
            const int64_t tile =
                bs_wave_tiles(std::min(8, map->R - g * 8), map->K, true, nullptr, unaligned) ? kBsTileWave : kBsTile;
            return (b.limited ? std::min<int64_t>(bs, b.min_len) : bs) / tile * tile;
        };
        auto tail_on_stream = [&](int g) {
            for (const auto& p : map->passes) {
                if (p.row0 / 8 != g) continue;
                if (p.ncols > 4 * kStreamGroups) return false;
                ApplyArgs t{};
                t.ncols = p.ncols;
                t.nrows = std::min(p.width, map->R - p.row0);
                for (int j = 0; j < p.ncols; j++) {
                    t.in_off[j] = in_off[p.col0 + j];
                    t.copy_off[j] = copy_off[p.col0 + j];
                }
                for (int r = 0; r < t.nrows; r++) t.out_off[r] = out_off[p.row0 + r];
                if (!stream_offsets(t, bs) || (p.row0 == 0 && !stream_copy_offsets(t, bs))) return false;
            }
            return true;
        };
        if (g_tune.stream && g_tune.frame_tail_fork != 0) {
            const int64_t rest = bs - cover_of(0);
            if (rest > 0 && rest < bs && (g_tune.frame_tail_fork == 2 || (rest >= 1024 && rest < 4096)) &&
                tail_on_stream(0)) {
                void* side = nullptr;
                const int rc = side_fork(map->device, stream, &side);
                if (rc) return rc;
                pst = static_cast<hipStream_t>(side);
                joiner.on = true;
            }
        }
        for (int g = 0; g * 8 < map->R && g_tune.stream; g++) {
            if (cover_of(g) < bs && !tail_on_stream(g)) continue;
            int brc = 0;
            b.copy_records = g == 0 ? 1 : 0;  // (recomputed from copy_off inside)
            bs_done[static_cast<size_t>(g)] =
                launch_bitslice(map, g * 8, std::min(8, map->R - g * 8), b, in_off.data(), out_off.data(), bs,
                                nstripes, st, &brc, g == 0 ? copy_off.data() : nullptr);
            if (brc) return brc;
        }
    }
    for (const auto& p : map->passes) {
        const int64_t done = bs_done[static_cast<size_t>(p.row0 / 8)];
        if (done >= bs) continue;
        const int64_t pbs = bs - done;  // this pass runs bytes [done, bs) of every fragment
        ApplyArgs a{};
        a.tables = map->d_tables + p.offset;
        a.in_base = in_base;
        a.in_stride = in_stride;
        a.out_base = out_base;
        a.out_stride = out_stride;
        a.copy_base = copy_base;
        a.copy_stride = copy_stride;
        a.bs = pbs;
        a.ncols = p.ncols;
        a.nrows = std::min(p.width, map->R - p.row0);
        a.accumulate = p.col0 > 0;
        auto rest = [&](int64_t len) { return static_cast<int32_t>(std::max<int64_t>(0, std::min(pbs, len - done))); };
        for (int j = 0; j < p.ncols; j++) {
            a.in_off[j] = in_off[p.col0 + j] + done;
            a.copy_off[j] = copy_off[p.col0 + j] < 0 ? -1 : copy_off[p.col0 + j] + done;
            a.in_len32[j] = rest(len_of(in_len, p.col0 + j));
            a.copy_len32[j] = rest(len_of(copy_len, p.col0 + j));
        }
        for (int r = 0; r < a.nrows; r++)
            a.out_len32[r] = rest(len_of(out_len, p.row0 + r));
        a.min_len = pbs;
        for (int j = 0; j < p.ncols; j++) {
            a.min_len = std::min<int64_t>(a.min_len, a.in_len32[j]);
            if (a.copy_off[j] >= 0) a.min_len = std::min<int64_t>(a.min_len, a.copy_len32[j]);
        }
        for (int r = 0; r < a.nrows; r++) a.min_len = std::min<int64_t>(a.min_len, a.out_len32[r]);
        a.limited = a.min_len < pbs ? 1 : 0;
        for (int r = 0; r < a.nrows; r++) a.out_off[r] = out_off[p.row0 + r] + done;
        Geometry g;
        int rc;
        if (g_tune.stream && p.ncols <= 4 * kStreamGroups && stream_offsets(a, pbs) &&
            (p.row0 != 0 || stream_copy_offsets(a, pbs))) {
            rc = launch_stream_pass(a, map->device, p.bytes, p.width, 1, false, pbs, nstripes, pst);
            if (rc) return rc;
            continue;
        }
        if (done > 0) return fail(ECAMD_EINVAL, "copy-through tail needs 32-bit stream offsets");
        rc = geometry(map->device, p.bytes, bs, nstripes, g);
        if (rc) return rc;
        a.ntiles = g.ntiles;
        a.tiles_per_stripe = g.tiles_per_stripe;
        dim3 grid(g.grid), block(g.threads);
        if (p.row0 == 0) {  // the first row group copies the inputs through
            switch (p.width) {
            case 2: hipLaunchKernelGGL((gf16_copy_apply_kernel<2>), grid, block, g.lds, pst, a); break;
            case 4: hipLaunchKernelGGL((gf16_copy_apply_kernel<4>), grid, block, g.lds, pst, a); break;
            default: hipLaunchKernelGGL((gf16_copy_apply_kernel<8>), grid, block, g.lds, pst, a); break;
            }
        } else {
            switch (p.width) {
            case 2: hipLaunchKernelGGL((gf16_apply_kernel<2, false, true, false>), grid, block, g.lds, pst, a); break;
            case 4: hipLaunchKernelGGL((gf16_apply_kernel<4, false, true, false>), grid, block, g.lds, pst, a); break;
            default: hipLaunchKernelGGL((gf16_apply_kernel<8, false, true, false>), grid, block, g.lds, pst, a); break;
            }
        }
        HIP_TRY(hipGetLastError());
    }
    if (joiner.on) {
        joiner.on = false;
        return side_join(map->device, stream);
    }
    return 0;
}

bool copy_aligned(const void* obj, const void* payload0, int64_t obj_stride, int64_t stripe_stride,
                  int64_t frag_stride, int64_t bs)
{
    return aligned16(obj) && aligned16(payload0) && obj_stride % 16 == 0 &&
           stripe_stride % 16 == 0 && frag_stride % 16 == 0 && bs % 16 == 0;
}

// Copy-through encode from objects whose k chunks of bs bytes start at unaligned object offsets
// (j*bs, bs even but not a multiple of 16) and may end early (objects shorter than k*bs): the
// payload side stays 16-byte aligned, the object side is read with unaligned 16-byte loads.
bool copy_aligned_payloads(const void* obj, const void* payload0, int64_t obj_stride,
                           int64_t stripe_stride, int64_t frag_stride, int64_t bs)
{
    return aligned16(obj) && aligned16(payload0) && obj_stride % 16 == 0 && stripe_stride % 16 == 0 &&
           frag_stride % 16 == 0 && bs % 2 == 0;
}

}  // namespace

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
namespace {
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
    if (slot < 0 || slot >= kStreamScratchSlots) return fail(ECAMD_EINVAL, "scratch slot %d", slot);
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
            return fail(ECAMD_EHIP, "side stream: %s", hipGetErrorString(rc));
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
    if (it == g_ctx.end() || !it->second.side) return fail(ECAMD_EHIP, "side_join without side_fork");
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

int rs_encode_copy(int k, int m, const void* obj, int64_t obj_stride, void* payload0,
                   int64_t stripe_stride, int64_t frag_stride, int64_t bs, int nstripes,
                   void* stream, int64_t obj_size, int64_t from, int64_t to)
{
    std::shared_ptr<RsEntry> e;
    int rc = rs_entry(0, k, m, nullptr, 0, -1, e);
    if (rc) return rc;
    if (!e->map || nstripes <= 0 || bs <= 0) return 0;
    if (obj_size < 0) obj_size = k * bs;
    if (obj_size > k * bs || !copy_aligned_payloads(obj, payload0, obj_stride, stripe_stride, frag_stride, bs))
        return fail(ECAMD_EINVAL, "copy-through encode needs 16-byte aligned objects and payloads");
    if (to < 0) to = bs;
    if (from < 0 || from % 16 || to > bs || from >= to || (to < bs && to % 16))
        return fail(ECAMD_EINVAL, "copy-through encode: bad range [%lld, %lld)", (long long)from, (long long)to);
    // bytes [from, to) of every payload: object chunk j from j*bs + from, payloads from + from
    const int64_t len = to - from;
    std::vector<int64_t> in_off, out_off, copy_off, in_len;
    for (int i : e->inputs) {
        in_off.push_back(static_cast<int64_t>(i) * bs + from);
        copy_off.push_back(static_cast<int64_t>(i) * frag_stride + from);
        in_len.push_back(std::min(len, std::max<int64_t>(
                                           0, std::min<int64_t>(bs, obj_size - static_cast<int64_t>(i) * bs) - from)));
    }
    for (int o : e->outputs) out_off.push_back(static_cast<int64_t>(o) * frag_stride + from);
    auto* p0 = static_cast<uint8_t*>(payload0);
    return map_apply_copy(*e, static_cast<const uint8_t*>(obj), obj_stride, in_off, p0,
                          stripe_stride, out_off, p0, stripe_stride, copy_off, len, nstripes, stream,
                          &in_len);
}

// LDS bytes of gf16_frame_crc_kernel for an RS(k, m) encode: the pass's split tables, the CRC image
// (byte tables for the first mb piece dwords) and the waves' state exchange.
size_t fused_crc_lds(int k, int m, int mb, bool nib)
{
    const int w = m <= 2 ? 2 : (m <= 4 ? 4 : 8);
    const int ns = 4 * ((k + 3) / 4) + w;
    return static_cast<size_t>(k) * (nib ? 64 : 512) * 2 * w + (static_cast<size_t>(crc_fused_words(mb)) + 8 * ns) * 4;
}

// rs_encode_copy with the payload CRC32 folded in (gf16_frame_crc_kernel): r0 of range r of
// payload f of stripe s lands in d_partial[(s*(k+m) + f)*q + r].  Returns ECAMD_EINVAL without
// launching when the shape does not fit the fused kernel (the caller then runs the split path).
int rs_encode_copy_crc(int k, int m, const void* obj, int64_t obj_stride, void* payload0,
                       int64_t stripe_stride, int64_t frag_stride, int64_t bs, int nstripes,
                       const uint32_t* d_img, uint32_t* d_partial, int q, void* stream, int mb, bool nib)
{
    constexpr int kThreads = 512;
    constexpr int64_t kTile = kThreads * 16;
    std::shared_ptr<RsEntry> e;
    int rc = rs_entry(0, k, m, nullptr, 0, -1, e);
    if (rc) return rc;
    if (!e->map || nstripes <= 0 || bs <= 0 || bs % kTile || q <= 0 || (bs / kTile) % q)
        return ECAMD_EINVAL;
    const ecamd_map* map = e->map.get();
    if (map->passes.size() != 1 || !copy_aligned(obj, payload0, obj_stride, stripe_stride, frag_stride, bs))
        return ECAMD_EINVAL;
    for (int j = 0; j < k; j++)
        if (e->inputs[j] != j) return ECAMD_EINVAL;
    for (int r = 0; r < m; r++)
        if (e->outputs[r] != k + r) return ECAMD_EINVAL;
    const auto& p = map->passes[0];
    ApplyArgs a{};
    a.tables = map->d_tables + (nib ? p.nib_offset : p.offset);
    a.in_base = static_cast<const uint8_t*>(obj);
    a.in_stride = obj_stride;
    a.out_base = static_cast<uint8_t*>(payload0);
    a.out_stride = stripe_stride;
    a.copy_base = static_cast<uint8_t*>(payload0);
    a.copy_stride = stripe_stride;
    a.bs = bs;
    a.ncols = k;
    a.nrows = m;
    for (int j = 0; j < k; j++) {
        a.in_off[j] = j * bs;
        a.copy_off[j] = j * frag_stride;
    }
    for (int r = 0; r < m; r++) a.out_off[r] = (k + r) * frag_stride;
    if (k > 4 * kStreamGroups || !stream_offsets(a, bs) || !stream_copy_offsets(a, bs)) return ECAMD_EINVAL;
    const int kg = (k + 3) / 4;
    const int ns = 4 * kg + p.width;
    if (mb != 1 && mb != 4) return ECAMD_EINVAL;
    if (nib && (!map->d_tables || p.nib_bytes == 0)) return ECAMD_EINVAL;
    const size_t lds = fused_crc_lds(k, m, mb, nib);
    if (lds != (nib ? p.nib_bytes : p.bytes) + (static_cast<size_t>(crc_fused_words(mb)) + 8 * ns) * 4)
        return ECAMD_EINVAL;
    if (lds > static_cast<size_t>(kLdsBytes)) return ECAMD_EINVAL;
    a.tiles_per_stripe = static_cast<uint32_t>(bs / kTile);
    a.ntiles = a.tiles_per_stripe * static_cast<uint32_t>(nstripes);
    FusedCrcArgs c{d_img, d_partial, q, static_cast<int>(bs / kTile) / q, k + m};
    const int64_t units = static_cast<int64_t>(nstripes) * q;
    const int wgs_knob = g_tune.frame_crc_wgs;
    const int want = wgs_knob > 0 ? wgs_knob : 2;
    const int wgs = std::max<int>(1, std::min<int>(want, kLdsBytes / static_cast<int>(lds)));
    const dim3 grid(static_cast<unsigned>(std::min<int64_t>(units, static_cast<int64_t>(cu_count(map->device)) * wgs)));
    const dim3 block(kThreads);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define ECAMD_FUSED(W, MB, NIB)                                                                                  \
    switch (kg) {                                                                                                \
    case 1: hipLaunchKernelGGL((gf16_frame_crc_kernel<W, 1, MB, NIB>), grid, block, lds, st, a, c); break;        \
    case 2: hipLaunchKernelGGL((gf16_frame_crc_kernel<W, 2, MB, NIB>), grid, block, lds, st, a, c); break;        \
    case 3: hipLaunchKernelGGL((gf16_frame_crc_kernel<W, 3, MB, NIB>), grid, block, lds, st, a, c); break;        \
    case 4: hipLaunchKernelGGL((gf16_frame_crc_kernel<W, 4, MB, NIB>), grid, block, lds, st, a, c); break;        \
    default: hipLaunchKernelGGL((gf16_frame_crc_kernel<W, 5, MB, NIB>), grid, block, lds, st, a, c); break;       \
    }
#define ECAMD_FUSED_W(W)                                    \
    if (nib) {                                              \
        if (mb == 4) { ECAMD_FUSED(W, 4, true) } else { ECAMD_FUSED(W, 1, true) }    \
    } else {                                                \
        if (mb == 4) { ECAMD_FUSED(W, 4, false) } else { ECAMD_FUSED(W, 1, false) }  \
    }
    if (p.width == 2) {
        ECAMD_FUSED_W(2)
    } else if (p.width == 4) {
        ECAMD_FUSED_W(4)
    } else {
        ECAMD_FUSED_W(8)
    }
#undef ECAMD_FUSED_W
#undef ECAMD_FUSED
    HIP_TRY(hipGetLastError());
    return 0;
}

namespace {

// The crc variant's prefetch and (one-wave form) occupancy for an m-output encode map with crc_pos
// flags -- shared by the launch and the build-time prebuild, so both name the same code object.
int crc_form_args(int m, int crc_pos, BsOcc& occ)
{
    occ = BsOcc{};
    if (!(crc_pos & 32)) return m <= 4 ? static_cast<int>(g_tune.frame_crc_prefetch) : 0;
    occ.wmin = g_tune.frame_crc_wave_wpe > 0 ? static_cast<int>(g_tune.frame_crc_wave_wpe) : m > 4 ? 2 : 3;
    occ.wmax = occ.wmin;
    // (5-8 outputs: no registers for a second input ahead)
    return m > 4 && g_tune.frame_crc_wave_pf == 3 ? 4 : static_cast<int>(g_tune.frame_crc_wave_pf);
}

// The crc variant of the bitsliced kernel for the encode map `coeff` (m x k, row-major; RS
// generator rows or a flat-XOR code's 0/1 parity masks) on `device`: see rs_encode_copy_crc_bs.
int encode_copy_crc_bs(int device, const std::vector<int>& coeff, int k, int m, const void* obj, int64_t obj_stride,
                       void* payload0, int64_t stripe_stride, int64_t frag_stride, int64_t bs, int nstripes,
                       const uint32_t* d_img, uint32_t* d_partial, int q, void* stream, int crc_pos, int64_t cover)
{
    const int mode = g_tune.bitslice;
    if (cover < 0) cover = bs;
    // crc_pos & 32: one-wave 4 KiB tiles in workgroups of (crc_pos >> 6) waves, per-tile partials
    // (tile-major, q unused); else more than 4 outputs fold every 16 KiB tile on its own
    // (bitslice.cpp fold_each), q = tiles
    const int cw = (crc_pos & 32) ? (crc_pos >> 6) & 15 : 0;
    const int64_t tile = cw ? kBsTileWave : kBsTile;
    if (!mode || m > kBsMaxR || k > kBsMaxK || cover % tile || cover <= 0 || cover > bs || nstripes <= 0 ||
        (!cw && (q <= 0 || (cover / kBsTile) % q || (m > 4 && q != cover / kBsTile))))
        return ECAMD_EINVAL;
    // whole payloads: the object chunks j*bs are 16-byte aligned; partial cover (objects that do not
    // fill k 16 KiB-multiple payloads): the object side is read with unaligned loads
    if (!(cover == bs ? copy_aligned(obj, payload0, obj_stride, stripe_stride, frag_stride, bs)
                      : copy_aligned_payloads(obj, payload0, obj_stride, stripe_stride, frag_stride, bs)))
        return ECAMD_EINVAL;
    ApplyArgs a{};
    a.in_base = static_cast<const uint8_t*>(obj);
    a.in_stride = obj_stride;
    a.out_base = static_cast<uint8_t*>(payload0);
    a.out_stride = stripe_stride;
    a.copy_base = static_cast<uint8_t*>(payload0);
    a.copy_stride = stripe_stride;
    a.ncols = k;
    a.nrows = m;
    for (int j = 0; j < k; j++) {
        a.in_off[j] = j * bs;
        a.copy_off[j] = j * frag_stride;
    }
    for (int r = 0; r < m; r++) a.out_off[r] = (k + r) * frag_stride;
    if (!stream_offsets(a, bs) || !stream_copy_offsets(a, bs) || k > 254) return ECAMD_EINVAL;
    std::shared_ptr<void> hold;
    // crc_pos: position sets (1, 2, 4) + 8 for the lane-shift fold (which 5-8 outputs always take)
    // + 16 for nibble piece tables
    // the crc variant keeps unaligned loads for object chunks at offsets that are not multiples of
    // 16: the realigned form measured no faster there (Swift segments 1.496 vs 1.486 ms, 4 MiB
    // objects 1.544 vs 1.542, profiles/r04_cover_ab2.log) and its larger register need spills at
    // some shift patterns (C3 objects 10 bytes long), which then fall back to the codec + CRC pass
    const uint32_t in_records = a.in_records;
    BsOcc occ{};
    const int prefetch = crc_form_args(m, crc_pos, occ);
    hipFunction_t fn = bitslice_function(device, coeff, m, k, 0, mode == 2, hold, true, crc_pos, false,
                                         nullptr, prefetch, nullptr, cw ? &occ : nullptr);
    if (!fn) return ECAMD_EINVAL;
    BsArgs b{};
    b.in_base = a.in_base;
    b.out_base = a.out_base;
    b.in_stride = a.in_stride;
    b.out_stride = a.out_stride;
    b.in_records = in_records;
    b.out_records = a.out_records;
    b.tiles_per_stripe = static_cast<uint32_t>(cover / tile);
    b.ntiles = b.tiles_per_stripe * static_cast<uint32_t>(nstripes);
    for (int j = 0; j < k; j++) {
        b.in_off[j] = a.in_off32[j];
        b.copy_idx[j] = static_cast<uint8_t>(j);
    }
    for (int r = 0; r < m; r++) b.out_off[r] = a.out_off32[r];
    b.copy_base = a.copy_base;
    b.copy_stride = a.copy_stride;
    b.copy_records = a.copy_records;
    b.copy_step = static_cast<uint32_t>(frag_stride);
    b.crc_img = d_img;
    b.crc_partial = d_partial;
    b.crc_q = q;
    b.crc_per = cw ? 0 : static_cast<int32_t>(cover / kBsTile / q);
    b.crc_nfrag = k + m;
    if (cw) {  // the first `big` workgroups: per tiles per wave, covering ~frame_crc_wave_big % of the
        // tiles; the rest one tile per wave
        const int64_t per = std::max<int64_t>(1, g_tune.frame_crc_wave_per);
        const int64_t big = per > 1 ? static_cast<int64_t>(b.ntiles) * g_tune.frame_crc_wave_big / 100 / (cw * per) : 0;
        b.crc_q = static_cast<int32_t>(big);
        b.crc_per = static_cast<int32_t>(per);
        const int64_t rest = static_cast<int64_t>(b.ntiles) - big * per * cw;
        const int64_t grid = big + (rest + cw - 1) / cw;
        return bitslice_launch(fn, b, static_cast<int>(grid), static_cast<hipStream_t>(stream), hold, 64 * cw,
                               cap_lds(fn, static_cast<int>(g_tune.frame_crc_per_cu)));
    }
    const int64_t units = static_cast<int64_t>(nstripes) * q;
    // one work unit per workgroup by default: the dispatcher hands the next unit to whichever CU
    // frees a slot, which balances units better than a grid-stride loop over resident workgroups
    const int wgs = static_cast<int>(g_tune.frame_crc_bs_wgs);
    const int grid = static_cast<int>(
        wgs > 0 ? std::min<int64_t>(units, static_cast<int64_t>(cu_count(device)) * wgs) : units);
    return bitslice_launch(fn, b, grid, static_cast<hipStream_t>(stream), hold, 256,
                           cap_lds(fn, static_cast<int>(g_tune.frame_crc_per_cu)));
}

}  // namespace

int rs_encode_copy_crc_bs(int k, int m, const void* obj, int64_t obj_stride, void* payload0,
                          int64_t stripe_stride, int64_t frag_stride, int64_t bs, int nstripes,
                          const uint32_t* d_img, uint32_t* d_partial, int q, void* stream, int crc_pos,
                          int64_t cover)
{
    if (!g_tune.bitslice || m > kBsMaxR || k > kBsMaxK) return ECAMD_EINVAL;
    std::shared_ptr<RsEntry> e;
    int rc = rs_entry(0, k, m, nullptr, 0, -1, e);
    if (rc) return rc;
    if (!e->map) return ECAMD_EINVAL;
    for (int j = 0; j < k; j++)
        if (e->inputs[j] != j) return ECAMD_EINVAL;
    for (int r = 0; r < m; r++)
        if (e->outputs[r] != k + r) return ECAMD_EINVAL;
    return encode_copy_crc_bs(e->map->device, e->map->coeff, k, m, obj, obj_stride, payload0, stripe_stride,
                              frag_stride, bs, nstripes, d_img, d_partial, q, stream, crc_pos, cover);
}

int xor_encode_copy_crc_bs(const uint32_t* masks, int k, int m, const void* obj, int64_t obj_stride, void* payload0,
                           int64_t stripe_stride, int64_t frag_stride, int64_t bs, int nstripes,
                           const uint32_t* d_img, uint32_t* d_partial, int q, void* stream, int crc_pos,
                           int64_t cover)
{
    int dev = 0;
    int rc = ensure_device(&dev);
    if (rc) return rc;
    if (!masks || !g_tune.bitslice || m > kBsMaxR || k > kBsMaxK) return ECAMD_EINVAL;
    // a flat-XOR code as a GF(2^16) matrix of 0 / 1: the bitsliced network of a coefficient 1 is the
    // identity on the bit planes, so the network is the parity masks' XORs
    std::vector<int> coeff(static_cast<size_t>(m) * k, 0);
    for (int r = 0; r < m; r++)
        for (int j = 0; j < k; j++) coeff[static_cast<size_t>(r) * k + j] = (masks[r] >> j) & 1u;
    return encode_copy_crc_bs(dev, coeff, k, m, obj, obj_stride, payload0, stripe_stride, frag_stride, bs, nstripes,
                              d_img, d_partial, q, stream, crc_pos, cover);
}

int xor_encode_copy(const uint32_t* masks, int k, int m, const void* obj, int64_t obj_stride, void* payload0,
                    int64_t stripe_stride, int64_t frag_stride, int64_t bs, int64_t cover, int nstripes, void* stream)
{
    int rc = ensure_device(nullptr);
    if (rc) return rc;
    if (nstripes <= 0 || cover <= 0) return 0;
    if (!masks || k <= 0 || k > 32 || m <= 0 || cover > bs || cover % 4096 || !aligned16(obj) || obj_stride % 16 ||
        !aligned16(payload0) || stripe_stride % 16 || frag_stride % 16)
        return ECAMD_EINVAL;
    std::vector<int64_t> in_off(static_cast<size_t>(k)), copy_off(static_cast<size_t>(k)), out_off(static_cast<size_t>(m));
    for (int j = 0; j < k; j++) {
        in_off[static_cast<size_t>(j)] = static_cast<int64_t>(j) * bs;
        copy_off[static_cast<size_t>(j)] = static_cast<int64_t>(j) * frag_stride;
    }
    for (int r = 0; r < m; r++) out_off[static_cast<size_t>(r)] = static_cast<int64_t>(k + r) * frag_stride;
    ApplyArgs a{};
    a.in_base = static_cast<const uint8_t*>(obj);
    a.in_stride = obj_stride;
    a.out_base = static_cast<uint8_t*>(payload0);
    a.out_stride = stripe_stride;
    a.copy_base = static_cast<uint8_t*>(payload0);
    a.copy_stride = stripe_stride;
    return launch_xor<false>(masks, m, k, a, in_off.data(), out_off.data(), cover, nstripes,
                             static_cast<hipStream_t>(stream), copy_off.data());
}

namespace {

// The decode-join of a prepared map (rs_decode_join, xor_decode_join): e's outputs are data fragments,
// computed into their object chunks; its data inputs are copied there as they stream through.
int decode_join_entry(const RsEntry& e, int k, const void* payload0, int64_t stripe_stride, int64_t frag_stride,
                      void* obj, int64_t obj_stride, int64_t bs, int nstripes, void* stream, int64_t obj_size)
{
    const RsEntry* ep = &e;
    if (!ep->map || nstripes <= 0 || bs <= 0)
        return fail(ECAMD_EINVAL, "decode-join needs at least one missing data fragment");
    if (obj_size < 0) obj_size = k * bs;
    if (obj_size > k * bs || !copy_aligned_payloads(obj, payload0, obj_stride, stripe_stride, frag_stride, bs))
        return fail(ECAMD_EINVAL, "decode-join needs 16-byte aligned objects and payloads");
    // object chunk j = [j*bs, j*bs + len_j): shorter (or empty) past the object's end
    auto chunk = [&](int j) {
        return std::max<int64_t>(0, std::min<int64_t>(bs, obj_size - static_cast<int64_t>(j) * bs));
    };
    std::vector<int64_t> in_off, out_off, copy_off, out_len, copy_len;
    for (int i : ep->inputs) {
        in_off.push_back(static_cast<int64_t>(i) * frag_stride);
        copy_off.push_back(i < k ? static_cast<int64_t>(i) * bs : -1);  // parity is not copied
        copy_len.push_back(i < k ? chunk(i) : bs);
    }
    for (int o : ep->outputs) {
        out_off.push_back(static_cast<int64_t>(o) * bs);
        out_len.push_back(chunk(o));
    }
    auto* ob = static_cast<uint8_t*>(obj);
    return map_apply_copy(*ep, static_cast<const uint8_t*>(payload0), stripe_stride, in_off, ob,
                          obj_stride, out_off, ob, obj_stride, copy_off, bs, nstripes, stream, nullptr,
                          &out_len, &copy_len);
}

}  // namespace

int rs_decode_join(int k, int m, const int* missing, const void* payload0, int64_t stripe_stride,
                   int64_t frag_stride, void* obj, int64_t obj_stride, int64_t bs, int nstripes,
                   void* stream, int64_t obj_size)
{
    std::shared_ptr<RsEntry> e;
    int rc = rs_entry(1, k, m, missing, 0, -1, e);
    if (rc) return rc;
    return decode_join_entry(*e, k, payload0, stripe_stride, frag_stride, obj, obj_stride, bs, nstripes, stream,
                             obj_size);
}

int xor_decode_join(int k, const std::vector<int>& inputs, const std::vector<int>& outputs,
                    const std::vector<int>& coeff, const void* payload0, int64_t stripe_stride, int64_t frag_stride,
                    void* obj, int64_t obj_stride, int64_t bs, int nstripes, void* stream, int64_t obj_size)
{
    int dev = 0;
    int rc = ensure_device(&dev);
    if (rc) return rc;
    const size_t R = outputs.size(), K = inputs.size();
    if (R == 0 || K == 0 || coeff.size() != R * K) return fail(ECAMD_EINVAL, "xor decode-join: bad matrix");
    for (int o : outputs)
        if (o < 0 || o >= k) return fail(ECAMD_EINVAL, "xor decode-join: outputs must be data fragments");
    // cached like the RS maps (kind 3): the map's coefficient tables live on the device
    std::vector<int> key = {dev, 3, k, static_cast<int>(R), static_cast<int>(K), 0};
    key.insert(key.end(), inputs.begin(), inputs.end());
    key.insert(key.end(), outputs.begin(), outputs.end());
    key.insert(key.end(), coeff.begin(), coeff.end());
    std::shared_ptr<RsEntry> e;
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        auto it = g_cache.find(key);
        if (it != g_cache.end()) {
            g_lru.splice(g_lru.begin(), g_lru, it->second.lru);
            e = it->second.entry;
        }
    }
    if (!e) {
        e = std::make_shared<RsEntry>();
        e->inputs = inputs;
        e->outputs = outputs;
        ecamd_map* mp = nullptr;
        if ((rc = ecamd_map_create(coeff.data(), static_cast<int>(R), static_cast<int>(K), &mp))) return rc;
        e->map.reset(mp);
        std::lock_guard<std::mutex> lk(g_cache_mu);
        cache_insert(key, e);
    }
    return decode_join_entry(*e, k, payload0, stripe_stride, frag_stride, obj, obj_stride, bs, nstripes, stream,
                             obj_size);
}

}  // namespace ecamd

namespace ecamd {

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
    if (e != hipSuccess) return fail(ECAMD_EHIP, "hipEventRecord: %s", hipGetErrorString(e));
    return 0;
}

}  // namespace ecamd

namespace ecamd {

int xor_apply_list(const uint32_t* masks, int R, int K, void* base, int64_t stripe_stride,
                   const int64_t* in_off, const int64_t* out_off, int64_t blocksize, int nstripes,
                   const int32_t* d_list, void* stream)
{
    if (!masks || !in_off || !out_off || R <= 0 || K <= 0 || K > 32 || !d_list)
        return fail(ECAMD_EINVAL, "bad xor map R=%d K=%d", R, K);
    if (nstripes <= 0 || blocksize <= 0) return 0;
    ApplyArgs a{};
    a.in_base = static_cast<const uint8_t*>(base);
    a.out_base = static_cast<uint8_t*>(base);
    a.in_stride = a.out_stride = stripe_stride;
    a.stripe_list = d_list;
    return launch_xor<false>(masks, R, K, a, in_off, out_off, blocksize, nstripes,
                             static_cast<hipStream_t>(stream));
}

}  // namespace ecamd

extern "C" {

int ecamd_init(void) { return ensure_device(nullptr); }

int ecamd_map_cache_stats(int64_t* entries, int64_t* bytes, int64_t* limit)
{
    std::lock_guard<std::mutex> lk(g_cache_mu);
    if (entries) *entries = static_cast<int64_t>(g_cache.size());
    if (bytes) *bytes = static_cast<int64_t>(g_cache_bytes);
    if (limit) *limit = static_cast<int64_t>(kCacheBytes);
    return 0;
}

int ecamd_tune(const char* key, int value)
{
    if (!key) return fail(ECAMD_EINVAL, "null key");
    const TuneSet r = tune_set(g_tune, key, value);  // the knobs and their rules: host/tune_knobs.def
    if (!r.knob) return fail(ECAMD_EINVAL, "unknown tuning key %s", key);
    if (!r.stored) return fail(ECAMD_EINVAL, "%s must be %s", key, r.knob->must);
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
    if (!dev) return fail(ECAMD_EINVAL, "null device pointer");
    HIP_TRY(hipGetDevice(dev));
    return 0;
}

int ecamd_set_device(int dev)
{
    HIP_TRY(hipSetDevice(dev));
    return 0;
}

const char* ecamd_last_error(void) { return g_err.c_str(); }

int ecamd_map_create(const int* coeff, int R, int K, ecamd_map** out)
{
    int dev = 0;
    int rc = ensure_device(&dev);
    if (rc) return rc;
    if (!coeff || !out || R <= 0 || K <= 0) return fail(ECAMD_EINVAL, "bad map R=%d K=%d", R, K);
    std::vector<int> c(coeff, coeff + static_cast<size_t>(R) * K);
    for (int& v : c) v &= 0xffff;
    auto passes = plan_passes(R, K);
    size_t total = passes.back().offset + passes.back().bytes;
    for (auto& p : passes) {
        p.nib_offset = total;
        p.nib_bytes = static_cast<size_t>(p.ncols) * 64 * 2 * p.width;
        total += p.nib_bytes;
    }
    std::vector<uint8_t> img(total);
    for (const auto& p : passes) {
        auto t = build_split_tables(c, R, K, p.row0, p.width, p.col0, p.ncols);
        std::memcpy(img.data() + p.offset, t.data(), t.size());
        auto n = build_nibble_tables(c, R, K, p.row0, p.width, p.col0, p.ncols);
        std::memcpy(img.data() + p.nib_offset, n.data(), n.size());
    }
    static std::atomic<uint64_t> next_serial{0};
    auto* map = new ecamd_map();
    map->serial = next_serial.fetch_add(1, std::memory_order_relaxed) + 1;
    map->device = dev;
    map->R = R;
    map->K = K;
    map->passes = passes;
    map->coeff = c;
    if (hipMalloc(&map->d_tables, total) != hipSuccess) {
        delete map;
        return fail(ECAMD_ENOMEM, "hipMalloc(%zu) for tables failed", total);
    }
    if (hipMemcpy(map->d_tables, img.data(), total, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(map->d_tables);
        delete map;
        return fail(ECAMD_EHIP, "table upload failed");
    }
    *out = map;
    return 0;
}

void ecamd_map_destroy(ecamd_map* map)
{
    if (!map) return;
    if (map->d_tables) (void)hipFree(map->d_tables);
    delete map;
}

int ecamd_map_apply_strided(const ecamd_map* map, const void* in_base, int64_t in_stripe_stride,
                            const int64_t* in_off, void* out_base, int64_t out_stripe_stride,
                            const int64_t* out_off, int64_t blocksize, int nstripes, void* stream)
{
    int rc = ensure_device(nullptr);
    if (rc) return rc;
    if (!map || !in_off || !out_off) return fail(ECAMD_EINVAL, "null argument");
    if (nstripes <= 0 || blocksize <= 0) return 0;
    bool ok = aligned16(in_base) && aligned16(out_base) && (in_stripe_stride % 16) == 0 &&
              (out_stripe_stride % 16) == 0;
    for (int j = 0; j < map->K; j++) ok = ok && (in_off[j] % 16) == 0;
    for (int r = 0; r < map->R; r++) ok = ok && (out_off[r] % 16) == 0;
    if (!ok) return fail(ECAMD_EINVAL, "fragment addresses must be 16-byte aligned");
    ApplyArgs a{};
    a.in_base = static_cast<const uint8_t*>(in_base);
    a.out_base = static_cast<uint8_t*>(out_base);
    a.in_stride = in_stripe_stride;
    a.out_stride = out_stripe_stride;
    return launch_gf16<false>(map, a, in_off, out_off, blocksize, nstripes,
                              static_cast<hipStream_t>(stream));
}

}  // extern "C"

namespace {
std::atomic<long long> g_small_crc_launches{0};

// The fused small-launch CRC image of (dev, machine, lane bytes G) (host/crc.hpp build_small_crc_image).
int small_crc_image(int dev, bool legacy, int G, const uint32_t** out)
{
    static std::mutex mu;
    static auto& images = *new std::map<std::tuple<int, bool, int>, uint32_t*>();  // never freed: no HIP call at exit
    std::lock_guard<std::mutex> lk(mu);
    auto it = images.find({dev, legacy, G});
    if (it == images.end()) {
        const std::vector<uint32_t> w = build_small_crc_image(CrcMachine(legacy), G);
        if (w.size() != static_cast<size_t>(small_crc_words(G))) return fail(ECAMD_EINVAL, "small CRC image layout");
        uint32_t* d = nullptr;
        HIP_TRY(hipMalloc(&d, w.size() * sizeof(uint32_t)));
        HIP_TRY(hipMemcpy(d, w.data(), w.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        it = images.emplace(std::make_tuple(dev, legacy, G), d).first;
    }
    *out = it->second;
    return 0;
}
}  // namespace

extern "C" {

int ecamd_map_apply_strided_crc(const ecamd_map* map, const void* in_base, const int64_t* in_off, void* out_base,
                                const int64_t* out_off, int64_t blocksize, int legacy, uint32_t* crc_out,
                                void* stream)
{
    int dev = 0;
    int rc = ensure_device(&dev);
    if (rc) return rc;
    if (!map || !in_off || !out_off || !crc_out) return fail(ECAMD_EINVAL, "null argument");
    if (blocksize <= 0) return 1;
    bool ok = aligned16(in_base) && aligned16(out_base);
    for (int j = 0; j < map->K; j++) ok = ok && (in_off[j] % 16) == 0;
    for (int r = 0; r < map->R; r++) ok = ok && (out_off[r] % 16) == 0;
    if (!ok) return fail(ECAMD_EINVAL, "fragment addresses must be 16-byte aligned");
    // one pass over every input and output row (the small kernel's single launch)
    if (map->passes.size() != 1 || map->K + map->R > 64) return 1;
    const auto& p = map->passes[0];
    if (p.col0 != 0 || p.ncols != map->K || p.row0 != 0 || std::min(p.width, map->R) != map->R) return 1;
    ApplyArgs a{};
    a.in_base = static_cast<const uint8_t*>(in_base);
    a.out_base = static_cast<uint8_t*>(out_base);
    a.tables = map->d_tables + p.offset;
    a.bs = blocksize;
    a.ncols = p.ncols;
    a.nrows = map->R;
    for (int j = 0; j < p.ncols; j++) a.in_off[j] = in_off[j];
    for (int r = 0; r < a.nrows; r++) a.out_off[r] = out_off[r];
    if (!small_launch(a, blocksize, 1)) return 1;
    SmallCrcReq req{};
    req.out = crc_out;
    req.legacy = legacy != 0;
    if ((rc = small_crc_image(dev, req.legacy, 2, &req.img[0])) || (rc = small_crc_image(dev, req.legacy, 4, &req.img[1])))
        return rc;
    StreamUse use(dev, stream);
    const size_t wgs = static_cast<size_t>((blocksize + 511) / 512 + 1);  // >= the launch's workgroups
    if ((rc = stream_scratch(dev, stream, kSmallCrcScratchSlot, 16 + static_cast<size_t>(map->K + map->R) * wgs,
                             &req.part)))
        return rc;
    rc = launch_small(a, p, blocksize, 1, map->d_tables, map->serial, static_cast<hipStream_t>(stream), &req, true,
                      true);
    if (rc == 0) g_small_crc_launches.fetch_add(1, std::memory_order_relaxed);
    return rc == ECAMD_EINVAL ? 1 : rc;
}

int ecamd_xor_apply_strided_crc(const uint32_t* masks, int R, int K, const void* in_base, const int64_t* in_off,
                                void* out_base, const int64_t* out_off, int64_t blocksize, int legacy,
                                uint32_t* crc_out, void* stream)
{
    int dev = 0;
    int rc = ensure_device(&dev);
    if (rc) return rc;
    if (!masks || !in_off || !out_off || !crc_out || R <= 0 || K <= 0 || K > 32)
        return fail(ECAMD_EINVAL, "bad xor map R=%d K=%d", R, K);
    if (blocksize <= 0 || R > kMaxRows || K + R > 64) return 1;  // one launch of at most 8 outputs
    bool ok = aligned16(in_base) && aligned16(out_base);
    for (int j = 0; j < K; j++) ok = ok && (in_off[j] % 16) == 0;
    for (int r = 0; r < R; r++) ok = ok && (out_off[r] % 16) == 0;
    if (!ok) return fail(ECAMD_EINVAL, "fragment addresses must be 16-byte aligned");
    ApplyArgs a{};
    a.in_base = static_cast<const uint8_t*>(in_base);
    a.out_base = static_cast<uint8_t*>(out_base);
    a.bs = blocksize;
    a.ncols = K;
    a.nrows = R;
    for (int j = 0; j < K; j++) a.in_off[j] = in_off[j];
    for (int r = 0; r < R; r++) {
        a.out_off[r] = out_off[r];
        a.masks[r] = masks[r];
    }
    if (!small_launch(a, blocksize, 1)) return 1;
    SmallCrcReq req{};
    req.out = crc_out;
    req.legacy = legacy != 0;
    if ((rc = small_crc_image(dev, req.legacy, 4, &req.img[1]))) return rc;
    StreamUse use(dev, stream);
    const size_t wgs = static_cast<size_t>((blocksize + 1023) / 1024 + 1);
    if ((rc = stream_scratch(dev, stream, kSmallCrcScratchSlot, 16 + static_cast<size_t>(K + R) * wgs, &req.part)))
        return rc;
    rc = launch_xor_small(a, blocksize, 1, static_cast<hipStream_t>(stream), true, &req, true);
    if (rc == 0) g_small_crc_launches.fetch_add(1, std::memory_order_relaxed);
    return rc == ECAMD_EINVAL ? 1 : rc;
}

long long ecamd_small_crc_launches(void) { return g_small_crc_launches.load(std::memory_order_relaxed); }

void ecamd_done_flag_arm(uint32_t* flag, uint32_t value) { t_done = DoneFlag{flag, value, false}; }

void ecamd_done_flag_arm_server(uint32_t* flag, uint32_t value, int mode)
{
    t_done = DoneFlag{flag, value, false};
    t_done.server = mode == 1 || mode == 2 ? mode : 0;
}

int ecamd_done_flag_taken(void)
{
    const int taken = t_done.served ? 2 : t_done.taken ? 1 : 0;
    t_done = DoneFlag{};
    return taken;
}

long long ecamd_small_server_posts(void) { return g_srv_posts.load(std::memory_order_relaxed); }
long long ecamd_small_server_launches(void) { return g_srv_launches.load(std::memory_order_relaxed); }
long long ecamd_small_server_rewrites(void) { return g_srv_rewrites.load(std::memory_order_relaxed); }
long long ecamd_small_server_stale_hits(void) { return g_srv_stale_hits.load(std::memory_order_relaxed); }

int ecamd_small_server_quiesce(void)
{
    SmallServer* sv = t_srv.s;
    if (!sv) return 0;
    // as server_post stops it for another kernel key: every workgroup exits at its next poll
    __atomic_store_n(&sv->box->stop, 1u, __ATOMIC_RELEASE);
    const hipError_t e = hipStreamSynchronize(sv->st);
    if (e != hipSuccess) return fail(ECAMD_EHIP, "small server: stop: %s", hipGetErrorString(e));
    __atomic_store_n(&sv->box->stop, 0u, __ATOMIC_RELEASE);
    sv->running = false;
    sv->cached[0].have = sv->cached[1].have = false;
    // workgroups that saw stop before the request sat it out while others ran and counted: the self-resetting
    // done and checksum counters may be left above 0 (as in ecamd_small_server_wait's relaunch)
    HIP_TRY(hipMemsetAsync(sv->scratch, 0, (64 + 16) * 4, sv->st));
    HIP_TRY(hipStreamSynchronize(sv->st));
    return 0;
}

int ecamd_small_server_wait(const uint32_t* flag, uint32_t value)
{
    SmallServer* sv = t_srv.s;
    if (!sv) return fail(ECAMD_EINVAL, "small server wait: no server on this thread");
    using clk = std::chrono::steady_clock;
    const auto deadline = clk::now() + std::chrono::seconds(10);
    auto check = clk::now() + std::chrono::microseconds(50);
    for (int i = 0;; i++) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == value) return 0;
        if ((i & 63) != 63) continue;
        const auto now = clk::now();
        if (now > check) {
            const hipError_t q = hipStreamQuery(sv->st);
            if (q == hipSuccess) {  // the server exited before this request: run it again, request pending
                if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == value) return 0;
                // Its workgroups leave one by one (each idle_ticks after its own last poll), so some of this
                // request's may have run and counted while the others were gone: the self-resetting done and
                // checksum counters then start the rerun above 0, a workgroup takes itself for the last one
                // early, and the flag (and the checksums) go out before every output.  Zero them first.
                HIP_TRY(hipMemsetAsync(sv->scratch, 0, (64 + 16) * 4, sv->st));
                const int rc = server_launch(sv, sv->key, sv->prev, true);
                if (rc) return rc;
                sv->last = now;
            } else if (q != hipErrorNotReady) {
                return fail(ECAMD_EHIP, "small server: %s", hipGetErrorString(q));
            }
            check = now + std::chrono::microseconds(50);
        }
        if (now > deadline) return fail(ECAMD_EHIP, "small server: no completion within 10 s");
    }
}

int ecamd_map_apply_ptrs(const ecamd_map* map, const void* const* d_in_ptrs, int in_row,
                         const int* in_col, void* const* d_out_ptrs, int out_row,
                         const int* out_col, int64_t blocksize, int nstripes, void* stream)
{
    int rc = ensure_device(nullptr);
    if (rc) return rc;
    if (!map || !d_in_ptrs || !d_out_ptrs || !in_col || !out_col)
        return fail(ECAMD_EINVAL, "null argument");
    if (nstripes <= 0 || blocksize <= 0) return 0;
    ApplyArgs a{};
    a.in_ptrs = reinterpret_cast<const uint8_t* const*>(d_in_ptrs);
    a.out_ptrs = reinterpret_cast<uint8_t* const*>(d_out_ptrs);
    a.in_stride = in_row;
    a.out_stride = out_row;
    std::vector<int64_t> io(in_col, in_col + map->K), oo(out_col, out_col + map->R);
    return launch_gf16<true>(map, a, io.data(), oo.data(), blocksize, nstripes,
                             static_cast<hipStream_t>(stream));
}

int ecamd_xor_apply_strided(const uint32_t* masks, int R, int K, const void* in_base,
                            int64_t in_stripe_stride, const int64_t* in_off, void* out_base,
                            int64_t out_stripe_stride, const int64_t* out_off, int64_t blocksize,
                            int nstripes, void* stream)
{
    int rc = ensure_device(nullptr);
    if (rc) return rc;
    if (!masks || !in_off || !out_off || R <= 0 || K <= 0 || K > 32)
        return fail(ECAMD_EINVAL, "bad xor map R=%d K=%d", R, K);
    if (nstripes <= 0 || blocksize <= 0) return 0;
    bool ok = aligned16(in_base) && aligned16(out_base) && (in_stripe_stride % 16) == 0 &&
              (out_stripe_stride % 16) == 0;
    for (int j = 0; j < K; j++) ok = ok && (in_off[j] % 16) == 0;
    for (int r = 0; r < R; r++) ok = ok && (out_off[r] % 16) == 0;
    if (!ok) return fail(ECAMD_EINVAL, "fragment addresses must be 16-byte aligned");
    ApplyArgs a{};
    a.in_base = static_cast<const uint8_t*>(in_base);
    a.out_base = static_cast<uint8_t*>(out_base);
    a.in_stride = in_stripe_stride;
    a.out_stride = out_stripe_stride;
    return launch_xor<false>(masks, R, K, a, in_off, out_off, blocksize, nstripes,
                             static_cast<hipStream_t>(stream));
}

int ecamd_xor_apply_ptrs(const uint32_t* masks, int R, int K, const void* const* d_in_ptrs,
                         int in_row, const int* in_col, void* const* d_out_ptrs, int out_row,
                         const int* out_col, int64_t blocksize, int nstripes, void* stream)
{
    int rc = ensure_device(nullptr);
    if (rc) return rc;
    if (!masks || !d_in_ptrs || !d_out_ptrs || !in_col || !out_col || R <= 0 || K <= 0 || K > 32)
        return fail(ECAMD_EINVAL, "bad xor map R=%d K=%d", R, K);
    if (nstripes <= 0 || blocksize <= 0) return 0;
    ApplyArgs a{};
    a.in_ptrs = reinterpret_cast<const uint8_t* const*>(d_in_ptrs);
    a.out_ptrs = reinterpret_cast<uint8_t* const*>(d_out_ptrs);
    a.in_stride = in_row;
    a.out_stride = out_row;
    std::vector<int64_t> io(in_col, in_col + K), oo(out_col, out_col + R);
    return launch_xor<true>(masks, R, K, a, io.data(), oo.data(), blocksize, nstripes,
                            static_cast<hipStream_t>(stream));
}

}  // extern "C"

namespace {
// decode_multi's fan-out: a heterogeneous batch runs one launch per erasure pattern, each over only that
// pattern's stripes -- short launches, each with its own ramp and tail.  With knob multi_streams N > 1
// the launches go round-robin to the caller's stream and N - 1 pool streams of the device, which wait
// for everything the caller's stream holds (fork event) and are waited for at the end (one event each):
// the dispatcher then overlaps one launch's tail with the next one's start.  The pool mutex is held from
// the fork to the join, so two callers never interleave their record / wait pairs on its events.
struct MultiPool {
    std::mutex mu;
    hipStream_t s[kMultiStreamsMax] = {};
    hipEvent_t done[kMultiStreamsMax] = {};
    hipEvent_t fork = nullptr;
    bool ready = false;
};

MultiPool& multi_pool(int dev)
{
    static std::mutex m;
    static auto& pools = *new std::map<int, MultiPool>();  // never destroyed: no HIP call at exit
    std::lock_guard<std::mutex> lk(m);
    return pools[dev];
}

// Creates the pool's streams and events once (pool.mu held); false when HIP refuses.
bool multi_pool_ready(MultiPool& p)
{
    if (p.ready) return true;
    bool ok = hipEventCreateWithFlags(&p.fork, hipEventDisableTiming) == hipSuccess;
    for (int i = 1; ok && i < kMultiStreamsMax; i++)
        ok = hipStreamCreateWithFlags(&p.s[i], hipStreamNonBlocking) == hipSuccess &&
             hipEventCreateWithFlags(&p.done[i], hipEventDisableTiming) == hipSuccess;
    (void)hipGetLastError();
    p.ready = ok;
    return ok;
}
}  // namespace

extern "C" {

int ecamd_rs_encode(int k, int m, void* base, int64_t stripe_stride, int64_t frag_stride,
                    int64_t blocksize, int nstripes, void* stream)
{
    std::shared_ptr<RsEntry> e;
    int rc = rs_entry(0, k, m, nullptr, 0, -1, e);
    if (rc) return rc;
    return rs_run(*e, base, stripe_stride, frag_stride, blocksize, nstripes, stream);
}

int ecamd_rs_decode(int k, int m, const int* missing, int rebuild_parity, void* base,
                    int64_t stripe_stride, int64_t frag_stride, int64_t blocksize, int nstripes,
                    void* stream)
{
    std::shared_ptr<RsEntry> e;
    int rc = rs_entry(1, k, m, missing, rebuild_parity ? 1 : 0, -1, e);
    if (rc) return rc;
    return rs_run(*e, base, stripe_stride, frag_stride, blocksize, nstripes, stream);
}

int ecamd_rs_decode_multi(int k, int m, const int* missing, int missing_stride,
                          int rebuild_parity, void* base, int64_t stripe_stride,
                          int64_t frag_stride, int64_t blocksize, int nstripes, void* stream)
{
    int dev = 0;
    int rc = ensure_device(&dev);
    if (rc) return rc;
    if (!missing || missing_stride < 1 || k <= 0 || m < 0 || k + m > 256)
        return fail(ECAMD_EINVAL, "bad decode_multi arguments");
    if (nstripes <= 0 || blocksize <= 0) return 0;
    if (!aligned16(base) || stripe_stride % 16 || frag_stride % 16)
        return fail(ECAMD_EINVAL, "fragment addresses must be 16-byte aligned");
    // Group stripes by erasure set (decode depends on the set, not the order of the list).
    std::map<std::vector<int>, std::vector<int>> groups;
    for (int s = 0; s < nstripes; s++) {
        const int* row = missing + static_cast<int64_t>(s) * missing_stride;
        std::vector<int> pat;
        for (int i = 0; i < missing_stride && row[i] >= 0; i++) {
            if (row[i] >= k + m) return fail(ECAMD_EINVAL, "stripe %d: missing index %d", s, row[i]);
            pat.push_back(row[i]);
        }
        std::sort(pat.begin(), pat.end());
        pat.erase(std::unique(pat.begin(), pat.end()), pat.end());
        if (static_cast<int>(pat.size()) > m)
            return fail(ECAMD_EINVAL, "stripe %d: %zu fragments missing > m=%d", s, pat.size(), m);
        groups[pat].push_back(s);
    }
    // The stream kernel walks each group's stripes of the strided layout through a stripe list
    // (one scalar load per tile); otherwise -- first-version kernels, k > 20 inputs, stripes
    // wider than 2 GiB -- one pointer table row (k+m fragment addresses) per stripe. Both are
    // laid out group by group.
    const int row = k + m;
    const bool use_list = g_tune.multi_list && g_tune.stream && g_tune.nt &&
                          k <= 4 * kStreamGroups &&
                          (row - 1) * frag_stride + blocksize < (int64_t(1) << 31);
    std::vector<uint8_t*> table;
    std::vector<int32_t> list;
    if (use_list) {
        list.reserve(nstripes);
        for (const auto& g : groups) list.insert(list.end(), g.second.begin(), g.second.end());
    } else {
        table.reserve(static_cast<size_t>(nstripes) * row);
        for (const auto& g : groups)
            for (int s : g.second)
                for (int f = 0; f < row; f++)
                    table.push_back(static_cast<uint8_t*>(base) + s * stripe_stride + f * frag_stride);
    }
    const size_t bytes = use_list ? list.size() * sizeof(int32_t) : table.size() * sizeof(uint8_t*);
    StagedUpload up;
    rc = up.begin(dev, stream, use_list ? static_cast<const void*>(list.data()) : table.data(), bytes);
    if (rc) return rc;
    auto* d_table = static_cast<uint8_t**>(up.dev);
    auto* d_list = static_cast<const int32_t*>(up.dev);
    // knob multi_streams: the launches of the patterns round-robin over the caller's stream and pool
    // streams forked from it (MultiPool); the pool streams join back before the upload is released
    int nonempty = 0;
    for (const auto& g : groups) nonempty += g.first.empty() ? 0 : 1;
    const int fan = use_list ? std::min<int>(static_cast<int>(g_tune.multi_streams), nonempty) : 1;
    MultiPool* pool = fan > 1 ? &multi_pool(dev) : nullptr;
    std::unique_lock<std::mutex> plk;
    if (pool) {
        plk = std::unique_lock<std::mutex>(pool->mu);
        if (!multi_pool_ready(*pool)) {
            plk.unlock();
            pool = nullptr;
        } else {
            bool ok = hipEventRecord(pool->fork, static_cast<hipStream_t>(stream)) == hipSuccess;
            for (int i = 1; ok && i < fan; i++) ok = hipStreamWaitEvent(pool->s[i], pool->fork, 0) == hipSuccess;
            if (!ok) {  // nothing launched on the pool yet: run everything on the caller's stream
                (void)hipGetLastError();
                plk.unlock();
                pool = nullptr;
            }
        }
    }
    int turn = 0;
    size_t at = 0;
    for (const auto& g : groups) {
        const int G = static_cast<int>(g.second.size());
        uint8_t** t = d_table + at * row;
        const int32_t* sl = d_list + at;
        at += static_cast<size_t>(G);
        if (g.first.empty()) continue;
        std::vector<int> list(g.first);
        list.push_back(-1);
        std::shared_ptr<RsEntry> e;
        rc = rs_entry(1, k, m, list.data(), rebuild_parity ? 1 : 0, -1, e);
        if (rc) break;
        if (e->outputs.empty()) continue;
        if (e->inputs.empty()) {
            for (int s : g.second)
                for (int o : e->outputs)
                    HIP_TRY(hipMemsetAsync(static_cast<uint8_t*>(base) + s * stripe_stride +
                                               o * frag_stride, 0, blocksize,
                                           static_cast<hipStream_t>(stream)));
            continue;
        }
        if (use_list) {
            std::vector<int64_t> in_off, out_off;
            for (int i : e->inputs) in_off.push_back(i * frag_stride);
            for (int o : e->outputs) out_off.push_back(o * frag_stride);
            ApplyArgs a{};
            a.in_base = static_cast<const uint8_t*>(base);
            a.out_base = static_cast<uint8_t*>(base);
            a.in_stride = a.out_stride = stripe_stride;
            a.stripe_list = sl;
            const int lane = pool ? turn++ % fan : 0;
            rc = launch_gf16<false>(e->map.get(), a, in_off.data(), out_off.data(), blocksize, G,
                                    lane ? pool->s[lane] : static_cast<hipStream_t>(stream));
        } else {
            rc = ecamd_map_apply_ptrs(e->map.get(), reinterpret_cast<const void* const*>(t), row,
                                      e->inputs.data(), reinterpret_cast<void* const*>(t), row,
                                      e->outputs.data(), blocksize, G, stream);
        }
        if (rc) break;
    }
    if (pool) {  // join: the caller's stream waits for every pool stream's launches (also after an error)
        for (int i = 1; i < fan; i++) {
            if (hipEventRecord(pool->done[i], pool->s[i]) != hipSuccess ||
                hipStreamWaitEvent(static_cast<hipStream_t>(stream), pool->done[i], 0) != hipSuccess) {
                (void)hipGetLastError();
                if (!rc) rc = fail(ECAMD_EHIP, "decode_multi: joining the pool streams failed");
            }
        }
        plk.unlock();
    }
    const int rc2 = up.end(stream);
    return rc ? rc : rc2;
}

int ecamd_scatter_fragments(const void* d_src, int64_t stripe_stride, int64_t frag_stride,
                            int64_t frag_len, int nfrags, int nstripes, const int* dst_dev,
                            void* const* d_dst, const int64_t* dst_stride, void* stream)
{
    int dev = 0;
    int rc = ensure_device(&dev);
    if (rc) return rc;
    if (!d_src || !dst_dev || !d_dst || !dst_stride || nfrags < 0 || nstripes < 0 || frag_len < 0)
        return fail(ECAMD_EINVAL, "bad scatter arguments");
    if (nfrags == 0 || nstripes == 0 || frag_len == 0) return 0;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    // Check every destination before anything is queued: a bad request copies nothing.
    for (int f = 0; f < nfrags; f++) {
        const int to = dst_dev[f];
        if (to < 0 || to >= ndev) return fail(ECAMD_EINVAL, "fragment %d: bad device %d", f, to);
        if (!d_dst[f] || dst_stride[f] < frag_len)
            return fail(ECAMD_EINVAL, "fragment %d: bad destination / stride", f);
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
                    return fail(ECAMD_EINVAL, "fragment %d: no peer path from device %d to %d", f, dev, to);
                }
                hipError_t e = hipDeviceEnablePeerAccess(to, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
                    int f = 0;
                    while (dst_dev[f] != to) f++;
                    return fail(ECAMD_EHIP, "fragment %d: hipDeviceEnablePeerAccess(%d -> %d): %s", f, dev,
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
            return fail(ECAMD_EHIP, "scatter fork: %s", hipGetErrorString(e));
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
                rc = fail(ECAMD_EHIP, "device %d lane: hipStreamWaitEvent: %s", to, hipGetErrorString(e));
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
                rc = fail(ECAMD_EHIP, "fragment %d -> device %d: hipMemcpy2DAsync: %s", f, to,
                          hipGetErrorString(e));
        }
        if (s != caller) {  // join: the caller's stream continues once this lane's copies landed
            hipEvent_t j = nullptr;
            hipError_t e = hipEventCreateWithFlags(&j, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventRecord(j, s);
            if (e == hipSuccess) e = hipStreamWaitEvent(caller, j, 0);
            if (j) joins.push_back(j);
            if (e != hipSuccess && rc == 0)
                rc = fail(ECAMD_EHIP, "device %d lane: join: %s", to, hipGetErrorString(e));
        }
        if (rc) break;
    }
    // events may be destroyed while pending: their resources go once they complete
    for (hipEvent_t j : joins) (void)hipEventDestroy(j);
    if (fork) (void)hipEventDestroy(fork);
    return rc;
}

int ecamd_rs_reconstruct(int k, int m, const int* missing, int dest, void* base,
                         int64_t stripe_stride, int64_t frag_stride, int64_t blocksize,
                         int nstripes, void* stream)
{
    std::shared_ptr<RsEntry> e;
    int rc = rs_entry(2, k, m, missing, 0, dest, e);
    if (rc) return rc;
    return rs_run(*e, base, stripe_stride, frag_stride, blocksize, nstripes, stream);
}

int ecamd_fill_splitmix(void* base, int64_t stripe_stride, int64_t frag_stride, int nfrags,
                        int64_t blocksize, int nstripes, int stripe0, uint64_t seed_base,
                        void* stream)
{
    int dev = 0;
    int rc = ensure_device(&dev);
    if (rc) return rc;
    if (!aligned16(base) || stripe_stride % 8 || frag_stride % 8)
        return fail(ECAMD_EINVAL, "fill: base must be 16-byte and strides 8-byte aligned");
    FillArgs f{static_cast<uint8_t*>(base), stripe_stride, frag_stride, blocksize, nfrags,
               nstripes, stripe0, seed_base};
    int64_t total = ((blocksize + 7) / 8) * nfrags * static_cast<int64_t>(nstripes);
    int64_t grid = std::min<int64_t>((total + 255) / 256, static_cast<int64_t>(cu_count(dev)) * 16);
    hipLaunchKernelGGL(splitmix_fill_kernel, dim3(static_cast<int>(std::max<int64_t>(grid, 1))),
                       dim3(256), 0, static_cast<hipStream_t>(stream), f);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ecamd_malloc(void** d_ptr, int64_t bytes)
{
    int rc = ensure_device(nullptr);
    if (rc) return rc;
    HIP_TRY(hipMalloc(d_ptr, static_cast<size_t>(bytes)));
    return 0;
}

int ecamd_malloc_host_writable(void** d_ptr, int64_t bytes)
{
    int rc = ensure_device(nullptr);
    if (rc) return rc;
    if (!d_ptr || bytes <= 0) return fail(ECAMD_EINVAL, "bad host-writable allocation");
    void* p = nullptr;
    // uncached on the GPU side: the kernel always sees what the host wrote last, no stale cache lines
    HIP_TRY(hipExtMallocWithFlags(&p, static_cast<size_t>(bytes), hipDeviceMallocUncached));
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) != hipSuccess || attr.hostPointer != p) {
        (void)hipGetLastError();
        (void)hipFree(p);
        return fail(ECAMD_EINVAL, "device memory is not host-accessible here (no large BAR)");
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
    int rc = ensure_device(nullptr);
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
    int rc = ensure_device(nullptr);
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

namespace {
// The coefficient map of an rs_vand operation: encode (missing NULL), decode (dest < 0) or
// single-destination reconstruct -- the same host planning rs_entry uses.
int rs_plan(int k, int m, const int* missing, int dest, int rebuild_parity, FragmentMap& fm)
{
    if (k <= 0 || m < 0 || k + m > 65536) return fail(ECAMD_EINVAL, "bad k=%d m=%d", k, m);
    std::vector<int> miss;
    if (missing)
        for (int i = 0; missing[i] > -1; i++) miss.push_back(missing[i]);
    const std::vector<int> G = rs_generator(k, m);
    if (G.empty()) return fail(ECAMD_EINVAL, "no generator for k=%d m=%d", k, m);
    if (!missing)
        fm = rs_encode_map(G, k, m);
    else if (dest < 0) {
        if (rs_decode_map(G, k, m, miss, rebuild_parity != 0, fm) != 0)
            return fail(ECAMD_EINVAL, "too many missing fragments (%zu > m=%d)", miss.size(), m);
    } else if (rs_reconstruct_map(G, k, m, miss, dest, fm) != 0)
        return fail(ECAMD_EINVAL, "cannot reconstruct %d", dest);
    return 0;
}

std::vector<int> group_rows(const FragmentMap& fm, int row0, int nrows)
{
    const size_t K = fm.inputs.size();
    return std::vector<int>(fm.coeff.begin() + static_cast<std::ptrdiff_t>(row0 * K),
                            fm.coeff.begin() + static_cast<std::ptrdiff_t>((row0 + nrows) * K));
}
}  // namespace

int ecamd_bitslice_prebuild(int k, int m, const int* missing, int dest, int rebuild_parity, const char* arch,
                            const char* dir)
{
    if (!arch || !dir) return fail(ECAMD_EINVAL, "null arch / dir");
    FragmentMap fm;
    int rc = rs_plan(k, m, missing, dest, rebuild_parity, fm);
    if (rc) return rc;
    const int R = static_cast<int>(fm.outputs.size()), K = static_cast<int>(fm.inputs.size());
    int built = 0;
    for (int row0 = 0; row0 < R && K > 0; row0 += 8) {
        const int nrows = std::min(8, R - row0);
        BsForm f;
        if (!bs_form(nrows, K, false, false, f)) continue;
        const int r = ecamd::bitslice_prebuild(group_rows(fm, row0, nrows), nrows, K, f.depth, false, 0, f.wave, nullptr,
                                               f.prefetch, f.occ, arch, dir, false, false, f.opts);
        if (r < 0) return fail(ECAMD_EHIP, "bitsliced prebuild failed (%d) for a %dx%d map", r, nrows, K);
        built += r;
    }
    return built;
}

extern "C++" {
namespace ecamd {
int crc_encode_prebuild(int k, int m, const uint32_t* masks, int crc_pos, const char* arch, const char* dir)
{
    if (!arch || !dir || k <= 0 || m <= 0 || m > kBsMaxR || k > kBsMaxK) return 0;
    std::vector<int> coeff(static_cast<size_t>(m) * k, 0);
    if (masks) {  // flat XOR: the 0 / 1 matrix of xor_encode_copy_crc_bs
        for (int r = 0; r < m; r++)
            for (int j = 0; j < k; j++) coeff[static_cast<size_t>(r) * k + j] = (masks[r] >> j) & 1u;
    } else {  // rs_vand: the generator's parity rows, as the encode map (rs_plan, no missing)
        FragmentMap fm;
        if (rs_plan(k, m, nullptr, -1, 0, fm)) return -1;
        coeff = group_rows(fm, 0, m);
    }
    BsOcc occ{};
    const int prefetch = crc_form_args(m, crc_pos, occ);
    return bitslice_prebuild(coeff, m, k, 0, true, crc_pos, false, nullptr, prefetch, occ, arch, dir);
}
}  // namespace ecamd
}  // extern "C++"

int ecamd_rs_kernel_form(int k, int m, const int* missing, int dest, int rebuild_parity, int64_t blocksize)
{
    int dev = 0;
    int rc = ensure_device(&dev);
    if (rc) return rc;
    FragmentMap fm;
    if ((rc = rs_plan(k, m, missing, dest, rebuild_parity, fm))) return rc;
    const int R = static_cast<int>(fm.outputs.size()), K = static_cast<int>(fm.inputs.size());
    // per row group of 8 outputs; the answer is the weakest: unavailable > compiling > bitsliced > tables
    auto rank = [](int form) { return form == ECAMD_FORM_UNAVAILABLE ? 3 : form == ECAMD_FORM_COMPILING ? 2
                                                                        : form == ECAMD_FORM_BITSLICED ? 1 : 0; };
    int form = ECAMD_FORM_TABLES;
    // one stripe of plain fragments this short takes gf16_small_kernel (launch_gf16's group_small): no
    // bitsliced launch, and no compile started for one
    if ((blocksize + 15) / 16 <= g_tune.small_chunks) return form;
    for (int row0 = 0; row0 < R && K > 0; row0 += 8) {
        const int nrows = std::min(8, R - row0);
        BsForm f;
        int g = ECAMD_FORM_TABLES;
        if (bs_form(nrows, K, false, false, f) && blocksize >= static_cast<int64_t>(bs_threads(f)) * 64) {
            std::shared_ptr<void> hold;
            int st = -1;
            (void)bitslice_function(dev, group_rows(fm, row0, nrows), nrows, K, f.depth, g_tune.bitslice == 2, hold,
                                    false, 0, f.wave, nullptr, f.prefetch, &st, &f.occ, false, false, f.opts);
            g = st == 1 ? ECAMD_FORM_BITSLICED : st == 0 ? ECAMD_FORM_COMPILING : ECAMD_FORM_UNAVAILABLE;
        }
        if (rank(g) > rank(form)) form = g;
    }
    return form;
}

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

int ecamd_bitslice_timeline(void* buf, unsigned records)
{
    if (records && !buf) return fail(ECAMD_EINVAL, "null timeline buffer");
    g_timeline_records.store(0, std::memory_order_relaxed);
    g_timeline.store(records ? static_cast<uint32_t*>(buf) : nullptr, std::memory_order_relaxed);
    g_timeline_records.store(records, std::memory_order_relaxed);
    return 0;
}

// what launch_bitslice counted for ecamd_check.hip
long long ecamd_check_fused_launches(void) { return g_check_fused.load(std::memory_order_relaxed); }
long long ecamd_locate_fused_launches(void) { return g_locate_fused.load(std::memory_order_relaxed); }
long long ecamd_xor_stream_launches(void) { return g_xor_stream_launches.load(std::memory_order_relaxed); }

}  // extern "C"
