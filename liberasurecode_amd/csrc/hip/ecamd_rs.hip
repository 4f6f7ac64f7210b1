// ecamd_rs.hip -- liberasurecode_rs_vand on the device: the one planner of its maps (rs_vand_plan),
// the bounded cache of prepared maps (rs_entry; check_map for ecamd_check.hip), and the C ABI over them:
// ecamd_rs_encode / decode / decode_multi (with its pool of streams) / reconstruct, the build-time
// ecamd_bitslice_prebuild, ecamd_rs_kernel_form and ecamd_map_cache_stats.  The cache is private to
// this file.
#include <algorithm>
#include <list>
#include <map>
#include <mutex>

#include "../host/gf16.hpp"
#include "../host/tune.hpp"
#include "ecamd_launch.hpp"

using namespace ecamd;

namespace {

// ---- cached liberasurecode_rs_vand maps ------------------------------------------------

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

// A new entry of (inputs, outputs, coeff) under `key`: its map made (none when a side is empty) and the
// entry inserted -- or, when another thread was first, that thread's.
int cache_add(const std::vector<int>& key, const std::vector<int>& inputs, const std::vector<int>& outputs,
              const std::vector<int>& coeff, std::shared_ptr<RsEntry>& out)
{
    auto e = std::make_shared<RsEntry>();
    e->inputs = inputs;
    e->outputs = outputs;
    if (!outputs.empty() && !inputs.empty()) {
        ecamd_map* mp = nullptr;
        const int rc = ecamd_map_create(coeff.data(), static_cast<int>(outputs.size()), static_cast<int>(inputs.size()), &mp);
        if (rc) return rc;
        e->map.reset(mp);
    }
    std::lock_guard<std::mutex> lk(g_cache_mu);
    cache_insert(key, e);
    out = e;
    return 0;
}

// The cached entry of `key`, most recently used again; null when there is none.
std::shared_ptr<RsEntry> cache_find(const std::vector<int>& key)
{
    std::lock_guard<std::mutex> lk(g_cache_mu);
    auto it = g_cache.find(key);
    if (it == g_cache.end()) return nullptr;
    g_lru.splice(g_lru.begin(), g_lru, it->second.lru);
    return it->second.entry;
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

// rs_vand_plan's kind of an rs_vand operation as the prebuild entry points name it: encode (missing
// NULL), decode (dest < 0) or single-destination reconstruct.
int plan_kind(const int* missing, int dest) { return !missing ? 0 : dest < 0 ? 1 : 2; }

std::vector<int> group_rows(const FragmentMap& fm, int row0, int nrows)
{
    const size_t K = fm.inputs.size();
    return std::vector<int>(fm.coeff.begin() + static_cast<std::ptrdiff_t>(row0 * K),
                            fm.coeff.begin() + static_cast<std::ptrdiff_t>((row0 + nrows) * K));
}

}  // namespace

namespace ecamd {

int rs_vand_plan(int kind, int k, int m, const int* missing, int dest, int rebuild, FragmentMap& fm)
{
    if (k <= 0 || m < 0 || k + m > 65536) return dev_fail(ECAMD_EINVAL, "bad k=%d m=%d", k, m);
    std::vector<int> miss;
    if (missing)
        for (int i = 0; missing[i] > -1; i++) miss.push_back(missing[i]);
    const std::vector<int> G = rs_generator(k, m);
    if (G.empty()) return dev_fail(ECAMD_EINVAL, "no generator for k=%d m=%d", k, m);
    if (kind == 0)
        fm = rs_encode_map(G, k, m);
    else if (kind == 1 || kind == 4) {  // 4, ecamd_rs_check: every surviving fragment beyond the first k
        if ((kind == 1 ? rs_decode_map(G, k, m, miss, rebuild != 0, fm) : rs_check_map(G, k, m, miss, fm)) != 0)
            return dev_fail(ECAMD_EINVAL, "too many missing fragments (%zu > m=%d)", miss.size(), m);
    } else if (rs_reconstruct_map(G, k, m, miss, dest, fm) != 0)
        return dev_fail(ECAMD_EINVAL, "cannot reconstruct %d", dest);
    return 0;
}

int rs_entry(int kind, int k, int m, const int* missing, int rebuild, int dest, std::shared_ptr<RsEntry>& out)
{
    int dev = 0;
    int rc = dev_ensure(&dev);
    if (rc) return rc;
    std::vector<int> key = {dev, kind, k, m, rebuild, dest};
    if (missing)
        for (int i = 0; missing[i] > -1; i++) key.push_back(missing[i]);
    if ((out = cache_find(key))) return 0;
    FragmentMap fm;
    if ((rc = rs_vand_plan(kind, k, m, missing, dest, rebuild, fm))) return rc;
    return cache_add(key, fm.inputs, fm.outputs, fm.coeff, out);
}

int xor_join_entry(int dev, int k, const std::vector<int>& inputs, const std::vector<int>& outputs,
                   const std::vector<int>& coeff, std::shared_ptr<RsEntry>& out)
{
    const size_t R = outputs.size(), K = inputs.size();
    std::vector<int> key = {dev, 3, k, static_cast<int>(R), static_cast<int>(K), 0};
    key.insert(key.end(), inputs.begin(), inputs.end());
    key.insert(key.end(), outputs.begin(), outputs.end());
    key.insert(key.end(), coeff.begin(), coeff.end());
    if ((out = cache_find(key))) return 0;
    return cache_add(key, inputs, outputs, coeff, out);
}

int check_map(int k, int m, const int* missing, CheckMap& out)
{
    std::shared_ptr<RsEntry> e;
    const int rc = rs_entry(4, k, m, missing, 0, -1, e);
    if (rc) return rc;
    out.inputs = &e->inputs;
    out.checked = &e->outputs;
    out.map = e->map.get();
    out.coeff = e->map ? &e->map->coeff : nullptr;
    out.pairs = &e->pairs;
    out.correct = &e->correct;
    out.hold = e;
    return 0;
}

}  // namespace ecamd

extern "C" {

int ecamd_map_cache_stats(int64_t* entries, int64_t* bytes, int64_t* limit)
{
    std::lock_guard<std::mutex> lk(g_cache_mu);
    if (entries) *entries = static_cast<int64_t>(g_cache.size());
    if (bytes) *bytes = static_cast<int64_t>(g_cache_bytes);
    if (limit) *limit = static_cast<int64_t>(kCacheBytes);
    return 0;
}

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
    int rc = dev_ensure(&dev);
    if (rc) return rc;
    if (!missing || missing_stride < 1 || k <= 0 || m < 0 || k + m > 256)
        return dev_fail(ECAMD_EINVAL, "bad decode_multi arguments");
    if (nstripes <= 0 || blocksize <= 0) return 0;
    if (!frags_aligned16(base, base, stripe_stride, frag_stride, nullptr, 0, nullptr, 0))
        return dev_fail(ECAMD_EINVAL, "fragment addresses must be 16-byte aligned");
    // Group stripes by erasure set (decode depends on the set, not the order of the list).
    std::map<std::vector<int>, std::vector<int>> groups;
    for (int s = 0; s < nstripes; s++) {
        const int* row = missing + static_cast<int64_t>(s) * missing_stride;
        std::vector<int> pat;
        for (int i = 0; i < missing_stride && row[i] >= 0; i++) {
            if (row[i] >= k + m) return dev_fail(ECAMD_EINVAL, "stripe %d: missing index %d", s, row[i]);
            pat.push_back(row[i]);
        }
        std::sort(pat.begin(), pat.end());
        pat.erase(std::unique(pat.begin(), pat.end()), pat.end());
        if (static_cast<int>(pat.size()) > m)
            return dev_fail(ECAMD_EINVAL, "stripe %d: %zu fragments missing > m=%d", s, pat.size(), m);
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
                if (!rc) rc = dev_fail(ECAMD_EHIP, "decode_multi: joining the pool streams failed");
            }
        }
        plk.unlock();
    }
    const int rc2 = up.end(stream);
    return rc ? rc : rc2;
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

int ecamd_bitslice_prebuild(int k, int m, const int* missing, int dest, int rebuild_parity, const char* arch,
                            const char* dir)
{
    if (!arch || !dir) return dev_fail(ECAMD_EINVAL, "null arch / dir");
    FragmentMap fm;
    int rc = rs_vand_plan(plan_kind(missing, dest), k, m, missing, dest, rebuild_parity, fm);
    if (rc) return rc;
    const int R = static_cast<int>(fm.outputs.size()), K = static_cast<int>(fm.inputs.size());
    int built = 0;
    for (int row0 = 0; row0 < R && K > 0; row0 += 8) {
        const int nrows = std::min(8, R - row0);
        BsForm f;
        if (!bs_form(nrows, K, false, false, f)) continue;
        const int r = ecamd::bitslice_prebuild(group_rows(fm, row0, nrows), nrows, K, f.depth, false, 0, f.wave, nullptr,
                                               f.prefetch, f.occ, arch, dir, false, false, f.opts);
        if (r < 0) return dev_fail(ECAMD_EHIP, "bitsliced prebuild failed (%d) for a %dx%d map", r, nrows, K);
        built += r;
    }
    return built;
}

int ecamd_rs_kernel_form(int k, int m, const int* missing, int dest, int rebuild_parity, int64_t blocksize)
{
    int dev = 0;
    int rc = dev_ensure(&dev);
    if (rc) return rc;
    FragmentMap fm;
    if ((rc = rs_vand_plan(plan_kind(missing, dest), k, m, missing, dest, rebuild_parity, fm))) return rc;
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

}  // extern "C"
