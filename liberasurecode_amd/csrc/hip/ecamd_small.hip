// ecamd_small.hip -- launches of a few KiB (gf16_small_kernel, xor_small_kernel): the fused checksum,
// the calling thread's completion flag and the resident small server (small_server_kernel, DESIGN.md
// §6), with the C ABI that drives them (ecamd_*_apply_strided_crc, ecamd_done_flag_*,
// ecamd_small_server_*).  The flag (t_done) and the thread's server (t_srv) are private to this file;
// ecamd_device.hip reaches it through small_launch / launch_small / launch_xor_small (ecamd_launch.hpp).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>

#include "../host/crc.hpp"
#include "../host/tune.hpp"
#include "ecamd_launch.hpp"
#include "ecamd_server_slots.hpp"

using namespace ecamd;

namespace {

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
    default: return dev_fail(ECAMD_EINVAL, "small server key %u", key);
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
            return dev_fail(ECAMD_EHIP, "small server: %s", hipGetErrorString(q));
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

std::atomic<long long> g_small_crc_launches{0};

// The fused small-launch CRC image of (dev, machine, lane bytes G) (host/crc.hpp build_small_crc_image).
int small_crc_image(int dev, bool legacy, int G, const uint32_t** out)
{
    static std::mutex mu;
    static auto& images = *new std::map<std::tuple<int, bool, int>, const uint32_t*>();  // never freed: no HIP call at exit
    std::lock_guard<std::mutex> lk(mu);
    auto it = images.find({dev, legacy, G});
    if (it == images.end()) {
        const std::vector<uint32_t> w = build_small_crc_image(CrcMachine(legacy), G);
        if (w.size() != static_cast<size_t>(small_crc_words(G))) return dev_fail(ECAMD_EINVAL, "small CRC image layout");
        const void* d = nullptr;
        if (const int rc = upload_table("small CRC image", w.data(), w.size() * sizeof(uint32_t), &d)) return rc;
        it = images.emplace(std::make_tuple(dev, legacy, G), static_cast<const uint32_t*>(d)).first;
    }
    *out = it->second;
    return 0;
}

}  // namespace

namespace ecamd {

// The fused checksum of a small launch (gf16_small_kernel CRC): the device image, where the CRCs go,
// the partials' scratch and the machine.
struct SmallCrcReq {
    const uint32_t* img[2];  // build_small_crc_image for 2- and 4-byte lanes
    uint32_t* out;
    uint32_t* part;
    bool legacy;
};

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

int launch_small(const ApplyArgs& a, const ecamd_map::Pass& p, int64_t bs, int nstripes, const uint8_t* tables,
                 uint64_t serial, hipStream_t st, const SmallCrcReq* crc, bool last, bool only)
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
int launch_xor_small(const ApplyArgs& a, int64_t bs, int nstripes, hipStream_t st, bool last, const SmallCrcReq* crc,
                     bool only)
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

}  // namespace ecamd

extern "C" {

int ecamd_map_apply_strided_crc(const ecamd_map* map, const void* in_base, const int64_t* in_off, void* out_base,
                                const int64_t* out_off, int64_t blocksize, int legacy, uint32_t* crc_out,
                                void* stream)
{
    int dev = 0;
    int rc = dev_ensure(&dev);
    if (rc) return rc;
    if (!map || !in_off || !out_off || !crc_out) return dev_fail(ECAMD_EINVAL, "null argument");
    if (blocksize <= 0) return 1;
    if (!frags_aligned16(in_base, out_base, 0, 0, in_off, map->K, out_off, map->R))  // one stripe: no strides
        return dev_fail(ECAMD_EINVAL, "fragment addresses must be 16-byte aligned");
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
    int rc = dev_ensure(&dev);
    if (rc) return rc;
    if (!masks || !in_off || !out_off || !crc_out || R <= 0 || K <= 0 || K > 32)
        return dev_fail(ECAMD_EINVAL, "bad xor map R=%d K=%d", R, K);
    if (blocksize <= 0 || R > kMaxRows || K + R > 64) return 1;  // one launch of at most 8 outputs
    if (!frags_aligned16(in_base, out_base, 0, 0, in_off, K, out_off, R))
        return dev_fail(ECAMD_EINVAL, "fragment addresses must be 16-byte aligned");
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
    if (e != hipSuccess) return dev_fail(ECAMD_EHIP, "small server: stop: %s", hipGetErrorString(e));
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
    if (!sv) return dev_fail(ECAMD_EINVAL, "small server wait: no server on this thread");
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
                return dev_fail(ECAMD_EHIP, "small server: %s", hipGetErrorString(q));
            }
            check = now + std::chrono::microseconds(50);
        }
        if (now > deadline) return dev_fail(ECAMD_EHIP, "small server: no completion within 10 s");
    }
}

}  // extern "C"
