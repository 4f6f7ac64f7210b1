// ecamd_device.hip -- applying a map: device discovery, fragment-map planning (row groups / column
// chunks sized to the 160 KiB LDS of a gfx950 CU), launch geometry, and the launchers of the stream,
// pointer-table, bitsliced and flat-XOR kernels behind ecamd_map_apply_* / ecamd_xor_apply_*
// (C ABI in include/ecamd.h).  Host code only.  What the other launch files take from here:
// ecamd_launch.hpp and ecamd_internal.hpp.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <numeric>

#include "../host/tables.hpp"
#include "../host/tune.hpp"
#include "ecamd_frame.hpp"
#include "ecamd_launch.hpp"

using namespace ecamd;

namespace {

struct DeviceInfo {
    int cus = 0;
    bool lds_attr_set = false;
};

std::mutex g_dev_mu;
int g_ndev = -1;
std::vector<DeviceInfo> g_dev;

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

// ecamd_bitslice_timeline's buffer (a development hook, measurement only): while set, the plain one-wave
// form runs its timeline form -- in every thread of the process, so the hook is for a tool that launches
// from one thread.  The two words are not set together: bs_form may still see the old count, and the
// launcher reads both again and hands the kernel a null buffer with a count of 0 whenever they disagree.
std::atomic<uint32_t*> g_timeline{nullptr};
std::atomic<uint32_t> g_timeline_records{0};

std::atomic<long long> g_check_fused{0};  // check-form launches enqueued by this process
std::atomic<long long> g_locate_fused{0};  // locate-form launches

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

constexpr int64_t kXorNarrowMin = 256 << 10;  // fragment bytes from which flat XOR takes 1 KiB tiles
std::atomic<long long> g_xor_stream_launches{0};  // xor_stream_kernel launches enqueued by this process

}  // namespace

namespace ecamd {

int dev_ensure(int* dev_out)
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
        return dev_fail(ECAMD_ENODEV, "liberasurecode_amd: no HIP device (MI355X) available; "
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

int dev_cu_count(int dev)
{
    std::lock_guard<std::mutex> lk(g_dev_mu);
    return g_dev[dev].cus;
}

int launch_stripes(int nstripes, uint64_t tiles_per_stripe, uint64_t slots, uint64_t limit)
{
    const uint64_t ntiles = tiles_per_stripe * static_cast<uint64_t>(nstripes);
    if (!limit || ntiles <= limit * slots) return nstripes;
    const uint64_t launches = (ntiles + limit * slots - 1) / (limit * slots);
    return static_cast<int>((static_cast<uint64_t>(nstripes) + launches - 1) / launches);
}

int geometry(int dev, size_t lds, int64_t bs, int nstripes, Geometry& g, int chunks, int max_threads, int max_wgs,
             int grid_mult)
{
    int wgs = lds ? static_cast<int>(std::min<size_t>(max_wgs, std::max<size_t>(1, kLdsBytes / lds))) : 8;
    int threads = lds ? std::min(1024, std::max(256, (1024 / wgs) / 64 * 64)) : 256;
    if (lds && g_tune.threads > 0) threads = g_tune.threads;
    threads = std::min(threads, max_threads);
    if (lds && g_tune.wgs_per_cu > 0) wgs = std::min<int>(g_tune.wgs_per_cu, std::max<size_t>(1, kLdsBytes / lds));
    int64_t span = static_cast<int64_t>(threads) * 16 * chunks;
    int64_t tps = (bs + span - 1) / span;
    int64_t nt = tps * nstripes;
    if (nt >= (1ll << 32)) return dev_fail(ECAMD_EINVAL, "batch too large: %lld tiles", (long long)nt);
    g.threads = threads;
    g.lds = lds;
    g.tiles_per_stripe = static_cast<uint32_t>(tps);
    g.ntiles = static_cast<uint32_t>(nt);
    int64_t grid = std::min<int64_t>(nt, static_cast<int64_t>(dev_cu_count(dev)) * wgs * std::max(1, grid_mult));
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

// One strided stream pass over a batch.  Within one launch the workgroups drift apart as they go
// and the tiles in flight spread over more and more of the batch, which costs HBM rate (C3, 2048
// stripes: one launch 5.34 TB/s, launches of 32 tiles per resident workgroup 5.85; 256 stripes
// spread over the span of 2048: 5.06-5.22, tools/span_probe.py, tools/slot_sweep.py,
// profiles/r02_{span_probe,slot_sweep}.log).  So a pass runs as launches of at most tiles_per_slot
// tiles per resident workgroup -- 32 for 4-output passes (C3 256 stripes: two launches, 0-2%
// faster than one), 64 for the others (C2 loses 1.5% at 32: its launches are short) -- each
// starting its workgroups in step again; 4-output launches of at most 64 tiles per slot take
// twice the resident workgroups (C3 +1.2-2.7%; C2 -7% and C5 -2-4% that way, so only there).
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

bool bs_wave_tiles(int nrows, int K, bool copy, bool* narrow, bool unaligned)
{
    const bool ok = !copy || g_tune.bs_wave_copy == 1 || (g_tune.bs_wave_copy == 2 && unaligned && g_tune.bs_realign);
    // 1-2 outputs (single-destination reconstruct, 1-2 lost): bitsliced when the map has at least
    // bs_narrow_min_k inputs (the LDS tables are K x 2 KiB there, and small at C2's k = 4)
    const bool few = nrows <= 2 && g_tune.bs_narrow_min_k > 0 && K >= g_tune.bs_narrow_min_k;
    const bool n = ok && g_tune.bs_wave >= 1 && (nrows >= g_tune.bs_wave_min_rows || few) && nrows <= 4;
    if (narrow) *narrow = n;
    return ok && (n || g_tune.bs_wave == 2);
}

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

// The bitsliced form (host/bitslice.hpp, hip/ecamd_jit.hip) of output rows row0 .. row0+nrows-1
// (5..8 of them) over ALL K <= 32 inputs -- whatever column chunks and row widths the LDS-table
// passes use -- on the whole 16 KiB tiles of every fragment; returns the bytes it covered (0: not
// taken -- shape, knob, or the kernel is still compiling); the LDS-table passes of those rows then
// run on the rest of each fragment only.
// Copy-through (copy_off non-null: the framed encode / decode-join of map_apply_copy): input j is
// also stored at copy_base + s*copy_stride + copy_off[j] (< 0: not copied) as it is loaded, and
// when base.limited (objects shorter than the k payloads) only the whole tiles below base.min_len
// are taken -- the LDS-table passes run the rest byte-exactly.
int64_t launch_bitslice(const ecamd_map* map, int row0, int nrows, const ApplyArgs& base,
                        const int64_t* in_off, const int64_t* out_off, int64_t bs, int nstripes,
                        hipStream_t st, int* rc, const int64_t* copy_off, const BsCheck* chk)
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
    const int64_t slots = static_cast<int64_t>(dev_cu_count(map->device)) * bitslice_waves_per_simd(nrows) * 4 * 64 / threads;
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

int64_t check_fused(int dev, const std::vector<int>& A, const Participants& p, int row0, int nrows, const StripeLayout& lay,
                    uint32_t* d_status, uint32_t* d_suspects, void* stream)
{
    const int K = p.K;
    if (nrows > kBsMaxR || K + nrows > kBsMaxK) return 0;
    ecamd_map syn;
    syn.device = dev;
    syn.R = nrows;
    syn.K = K + nrows;
    syn.coeff = syndrome_rows(A, K, row0, nrows);
    // the map's inputs: the K inputs, then the checked rows of this group
    const int64_t* chk_off = p.off + K + row0;
    const uint8_t* chk_bit = p.bit + K + row0;
    std::vector<int64_t> off(p.off, p.off + K);
    off.insert(off.end(), chk_off, chk_off + nrows);
    std::vector<uint8_t> frag_bits(p.bit, p.bit + K);
    frag_bits.insert(frag_bits.end(), chk_bit, chk_bit + nrows);
    ApplyArgs a{};
    a.in_base = lay.base;
    a.in_stride = lay.stripe_stride;
    const BsCheck chk{d_status, chk_bit, d_suspects, frag_bits.data()};
    int rc = 0;
    const int64_t cover = launch_bitslice(&syn, 0, nrows, a, off.data(), nullptr, lay.blocksize, lay.nstripes,
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
            return dev_fail(ECAMD_EINVAL, "stripe list on a non-stream launch");
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

template <bool PTRS>
int launch_xor(const uint32_t* masks, int R, int K, ApplyArgs base_args, const int64_t* in_off,
               const int64_t* out_off, int64_t bs, int nstripes, hipStream_t st, const int64_t* copy_off)
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
                if (!stream_copy_offsets(a, bs)) return dev_fail(ECAMD_EINVAL, "xor copy-through offsets");
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
                const int64_t slots = static_cast<int64_t>(dev_cu_count(dev)) * wgs;
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
                    return dev_fail(ECAMD_EINVAL, "stripe list on a non-stream xor launch");
                hipLaunchKernelGGL((xor_apply_kernel<8, PTRS>), dim3(g.grid), dim3(g.threads), 0, st,
                                   a);
            }
            HIP_TRY(hipGetLastError());
        }
    }
    return 0;
}

template int launch_gf16<false>(const ecamd_map*, ApplyArgs, const int64_t*, const int64_t*, int64_t, int, hipStream_t);
template int launch_gf16<true>(const ecamd_map*, ApplyArgs, const int64_t*, const int64_t*, int64_t, int, hipStream_t);
template int launch_xor<false>(const uint32_t*, int, int, ApplyArgs, const int64_t*, const int64_t*, int64_t, int,
                               hipStream_t, const int64_t*);
template int launch_xor<true>(const uint32_t*, int, int, ApplyArgs, const int64_t*, const int64_t*, int64_t, int,
                              hipStream_t, const int64_t*);

int xor_apply_list(const uint32_t* masks, int R, int K, void* base, int64_t stripe_stride,
                   const int64_t* in_off, const int64_t* out_off, int64_t blocksize, int nstripes,
                   const int32_t* d_list, void* stream)
{
    if (!masks || !in_off || !out_off || R <= 0 || K <= 0 || K > 32 || !d_list)
        return dev_fail(ECAMD_EINVAL, "bad xor map R=%d K=%d", R, K);
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

int ecamd_init(void) { return dev_ensure(nullptr); }

int ecamd_map_create(const int* coeff, int R, int K, ecamd_map** out)
{
    int dev = 0;
    int rc = dev_ensure(&dev);
    if (rc) return rc;
    if (!coeff || !out || R <= 0 || K <= 0) return dev_fail(ECAMD_EINVAL, "bad map R=%d K=%d", R, K);
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
        return dev_fail(ECAMD_ENOMEM, "hipMalloc(%zu) for tables failed", total);
    }
    if (hipMemcpy(map->d_tables, img.data(), total, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(map->d_tables);
        delete map;
        return dev_fail(ECAMD_EHIP, "table upload failed");
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
    int rc = dev_ensure(nullptr);
    if (rc) return rc;
    if (!map || !in_off || !out_off) return dev_fail(ECAMD_EINVAL, "null argument");
    if (nstripes <= 0 || blocksize <= 0) return 0;
    if (!frags_aligned16(in_base, out_base, in_stripe_stride, out_stripe_stride, in_off, map->K, out_off, map->R))
        return dev_fail(ECAMD_EINVAL, "fragment addresses must be 16-byte aligned");
    ApplyArgs a{};
    a.in_base = static_cast<const uint8_t*>(in_base);
    a.out_base = static_cast<uint8_t*>(out_base);
    a.in_stride = in_stripe_stride;
    a.out_stride = out_stripe_stride;
    return launch_gf16<false>(map, a, in_off, out_off, blocksize, nstripes,
                              static_cast<hipStream_t>(stream));
}

int ecamd_map_apply_ptrs(const ecamd_map* map, const void* const* d_in_ptrs, int in_row,
                         const int* in_col, void* const* d_out_ptrs, int out_row,
                         const int* out_col, int64_t blocksize, int nstripes, void* stream)
{
    int rc = dev_ensure(nullptr);
    if (rc) return rc;
    if (!map || !d_in_ptrs || !d_out_ptrs || !in_col || !out_col)
        return dev_fail(ECAMD_EINVAL, "null argument");
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
    int rc = dev_ensure(nullptr);
    if (rc) return rc;
    if (!masks || !in_off || !out_off || R <= 0 || K <= 0 || K > 32)
        return dev_fail(ECAMD_EINVAL, "bad xor map R=%d K=%d", R, K);
    if (nstripes <= 0 || blocksize <= 0) return 0;
    if (!frags_aligned16(in_base, out_base, in_stripe_stride, out_stripe_stride, in_off, K, out_off, R))
        return dev_fail(ECAMD_EINVAL, "fragment addresses must be 16-byte aligned");
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
    int rc = dev_ensure(nullptr);
    if (rc) return rc;
    if (!masks || !d_in_ptrs || !d_out_ptrs || !in_col || !out_col || R <= 0 || K <= 0 || K > 32)
        return dev_fail(ECAMD_EINVAL, "bad xor map R=%d K=%d", R, K);
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

int ecamd_bitslice_timeline(void* buf, unsigned records)
{
    if (records && !buf) return dev_fail(ECAMD_EINVAL, "null timeline buffer");
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
