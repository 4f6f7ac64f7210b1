// ecamd_xor_decode_masks.hip -- ecamd_xor_decode_masks (DESIGN.md "Decode from device masks"): the flat_xor_hd
// counterpart of ecamd_rs_decode_masks.  Rebuild the lost fragments of a batch in which every stripe lost
// a different set, the sets given as one mask word per stripe in DEVICE memory.
//
// A flat XOR code has no plan to work out on the device: the reference refuses hd or more lost fragments,
// so a code has at most 2952 recoverable patterns, and its whole decode is one table of 16-byte entries
// (ecamd_xor_masks_plan.hpp) found by the rank of the mask.  Two launches on the caller's stream, whatever
// the masks hold -- no host wait, no map, no compile:
//   xor_decode_masks_kernel  grid (tiles, stripe slots), grid-stride over both: a workgroup ranks its
//                            stripe's mask, loads the entry and streams the stripe's tiles as a
//                            mask-driven XOR; its first tile column writes d_result[s];
//   xor_masks_counts_kernel  with d_counts: the three counts, from the masks.
// T, the data kernel's tile, is 4096 bytes: 256 lanes of one 16-byte chunk per fragment.
#include <hip/hip_runtime.h>

#include <atomic>
#include <vector>

#include "ecamd.h"
#include "ecamd_apply.hpp"
#include "ecamd_host.h"
#include "ecamd_internal.hpp"
#include "ecamd_xor_masks_plan.hpp"

using namespace ecamd;

namespace {

typedef unsigned int v4u __attribute__((ext_vector_type(4)));

struct XorMasksArgs {
    uint8_t* base;  // fragment f of stripe s at base + s*stripe_stride + f*frag_stride
    const uint32_t* lost;
    const XorMasksEntry* table;
    uint32_t* result;  // may be null
    int64_t stripe_stride, frag_stride;
    int64_t len;  // bytes per fragment
    int32_t nstripes, k, n, hd, decode_parity;
};

// Output r accumulates the lane's chunk x of fragment f under the scalar mask bit f of src[r]: one v_bitop3
// per dword (acc ^ (x & m)), no branch.
__device__ __forceinline__ void xm_accumulate(v4u (&acc)[kXorMasksMaxOut], const uint32_t (&src)[kXorMasksMaxOut], uint32_t f, v4u x)
{
#pragma unroll
    for (int r = 0; r < kXorMasksMaxOut; r++) {
        const uint32_t msk = 0u - ((src[r] >> f) & 1u);  // wave-uniform
#pragma unroll
        for (int d = 0; d < 4; d++) acc[r][d] = xor_and(acc[r][d], x[d], msk);
    }
}

// No fragment has this index (k + m <= 26), so no source mask has its bit: the place of a group's
// lanes past the last fragment of U.
constexpr uint32_t kNoFrag = 31;

// The next four fragments of `rest` (scalar; their bits are taken out of it): their indices in f, the
// lane's chunk of each (xp: the chunk's place in fragment 0) in x, 128-bit non-temporal loads.  FULL: the
// caller knows that four are left, and the four loads are unconditional.  Otherwise, past the last set
// bit: kNoFrag and zeros, nothing loaded.
template <bool FULL>
__device__ __forceinline__ void xm_load_group(const uint8_t* xp, int64_t frag_stride, uint32_t& rest, uint32_t (&f)[4], v4u (&x)[4])
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        f[i] = kNoFrag;
        x[i] = v4u{0u, 0u, 0u, 0u};
        if (FULL || rest) {
            f[i] = static_cast<uint32_t>(__builtin_ctz(rest));
            rest &= rest - 1u;
            x[i] = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(xp + static_cast<int64_t>(f[i]) * frag_stride));
        }
    }
}

__device__ __forceinline__ void xm_accumulate_group(v4u (&acc)[kXorMasksMaxOut], const uint32_t (&src)[kXorMasksMaxOut],
                                                    const uint32_t (&f)[4], const v4u (&x)[4])
{
#pragma unroll
    for (int i = 0; i < 4; i++) xm_accumulate(acc, src, f[i], x[i]);
}

// One whole 16-byte chunk of one stripe: the fragments of U (the union of src[r], r < n_out) in groups of
// four, the next group's loads issued before this group's accumulates; then the n_out stores.  While
// four or more fragments are left the next group is four unconditional loads, so the wait in front of the
// accumulates is for this group alone (vmcnt(4)); only the last group, of one to three, is loaded under
// scalar branches, where the compiler must wait as if it were one load.
__device__ __forceinline__ void xm_chunk(uint8_t* xp, int64_t frag_stride, uint32_t U, const uint32_t (&src)[kXorMasksMaxOut],
                                         const uint32_t (&out)[kXorMasksMaxOut], int n_out)
{
    v4u acc[kXorMasksMaxOut];
#pragma unroll
    for (int r = 0; r < kXorMasksMaxOut; r++) acc[r] = v4u{0u, 0u, 0u, 0u};
    uint32_t rest = U, f[4], fn[4];
    v4u x[4], nxt[4];
    if (__builtin_popcount(rest) >= 4)
        xm_load_group<true>(xp, frag_stride, rest, f, x);
    else
        xm_load_group<false>(xp, frag_stride, rest, f, x);
    while (__builtin_popcount(rest) >= 4) {  // scalar
        xm_load_group<true>(xp, frag_stride, rest, fn, nxt);
        xm_accumulate_group(acc, src, f, x);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            f[i] = fn[i];
            x[i] = nxt[i];
        }
    }
    if (rest) {
        xm_load_group<false>(xp, frag_stride, rest, fn, nxt);
        xm_accumulate_group(acc, src, f, x);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            f[i] = fn[i];
            x[i] = nxt[i];
        }
    }
    xm_accumulate_group(acc, src, f, x);
#pragma unroll
    for (int r = 0; r < kXorMasksMaxOut; r++)
        if (r < n_out) __builtin_nontemporal_store(acc[r], reinterpret_cast<v4u*>(xp + static_cast<int64_t>(out[r]) * frag_stride));
}

// The last, partial chunk of a fragment (rem bytes, one lane of the stripe's last tile): byte by byte
// through load_tail / store_tail, so nothing at or past `len` is read or written; one fragment at a time.
__device__ __forceinline__ void xm_tail_chunk(uint8_t* xp, int64_t frag_stride, int rem, uint32_t U,
                                              const uint32_t (&src)[kXorMasksMaxOut], const uint32_t (&out)[kXorMasksMaxOut], int n_out)
{
    v4u acc[kXorMasksMaxOut];
#pragma unroll
    for (int r = 0; r < kXorMasksMaxOut; r++) acc[r] = v4u{0u, 0u, 0u, 0u};
    for (uint32_t rest = U; rest; rest &= rest - 1u) {
        const uint32_t f = static_cast<uint32_t>(__builtin_ctz(rest));
        const uint4 t = load_tail(xp + static_cast<int64_t>(f) * frag_stride, rem);
        xm_accumulate(acc, src, f, v4u{t.x, t.y, t.z, t.w});
    }
#pragma unroll
    for (int r = 0; r < kXorMasksMaxOut; r++)
        if (r < n_out)
            store_tail(xp + static_cast<int64_t>(out[r]) * frag_stride, make_uint4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]), rem);
}

// grid (tiles, stripe slots), grid-stride over both, as decode_masks_kernel.  Per stripe a workgroup
//   - reads the mask through readfirstlane, so its rank, the entry and everything selected by them
//     (offsets, predicates, loop counts) is scalar and all lanes take the same branches; a stripe with
//     nothing to write -- no loss, an unrecoverable one, lost parity alone without decode_parity --
//     costs that one word load (and the entry's, for the last kind);
//   - takes U, the union of the source masks of the outputs it writes, and walks its set bits in
//     groups of four: 128-bit non-temporal loads, the next group's issued before this group's
//     accumulates.  A fragment is loaded once per tile however many outputs it feeds, and accumulated
//     into output r under the scalar mask bit of src[r] (one v_bitop3 per dword, no branch);
//   - stores the outputs with 128-bit non-temporal stores.  The lost slots are written and never read;
//     nothing else is written.
// The workgroups of tile column 0 write the stripe's result word (every stripe is visited by exactly
// one of them).  No LDS, no atomics.
// At most two waves per SIMD -- two workgroups per CU, the residency xor_stream_kernel's grid gives it: the
// registers would allow seven, and at (10,6,4), 1 MiB fragments, 256 stripes, every stripe losing {0,1,2}, a cap
// of 2 took 0.54 ms against 0.57 ms without one (DESIGN.md "Decode from device masks").
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) xor_decode_masks_kernel(const XorMasksArgs a)
{
    const int64_t whole = a.len >> 4, chunks = (a.len + 15) >> 4;
    const int rem = static_cast<int>(a.len & 15);
    const bool reports = a.result != nullptr && blockIdx.x == 0 && threadIdx.x == 0;
    for (int s = static_cast<int>(blockIdx.y); s < a.nstripes; s += static_cast<int>(gridDim.y)) {
        const uint32_t L = __builtin_amdgcn_readfirstlane(a.lost[s]);
        if (L == 0u) {
            if (reports) a.result[s] = 0u;
            continue;
        }
        const int32_t rank = xor_masks_rank(a.n, a.hd, L);
        if (rank < 0) {
            if (reports) a.result[s] = 0x80000000u | static_cast<uint32_t>(__builtin_popcount(L));
            continue;
        }
        const uint32_t* ew = reinterpret_cast<const uint32_t*>(a.table + rank);
        const uint32_t head = __builtin_amdgcn_readfirstlane(ew[0]);
        uint32_t src[kXorMasksMaxOut], out[kXorMasksMaxOut];
        int n_out = 0;  // the entry's outputs, or with decode_parity 0 its leading ones below k
        uint32_t U = 0u;
#pragma unroll
        for (int r = 0; r < kXorMasksMaxOut; r++) {
            out[r] = (head >> (8 * (r + 1))) & 0xffu;
            src[r] = 0u;
            if (r < static_cast<int>(head & 0xffu) && (a.decode_parity || out[r] < static_cast<uint32_t>(a.k))) {
                src[r] = __builtin_amdgcn_readfirstlane(ew[1 + r]);
                n_out = r + 1;
            }
            U |= src[r];
        }
        if (reports) a.result[s] = static_cast<uint32_t>(n_out);
        if (n_out == 0) continue;
        uint8_t* xs = a.base + static_cast<int64_t>(s) * a.stripe_stride;
        for (int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; p < chunks;
             p += static_cast<int64_t>(gridDim.x) * 256) {
            uint8_t* xp = xs + p * 16;
            if (p < whole)
                xm_chunk(xp, a.frag_stride, U, src, out, n_out);
            else
                xm_tail_chunk(xp, a.frag_stride, rem, U, src, out, n_out);
        }
    }
}

// counts[0..2] = stripes left alone (result 0), rebuilt, unrecoverable, as masks_counts_kernel's -- from
// the masks, so that d_result may be null.  One workgroup; the three words are overwritten.
__global__ void __launch_bounds__(256) xor_masks_counts_kernel(const uint32_t* lost, int n, int k, int nfrag, int hd,
                                                               int decode_parity, uint32_t* counts)
{
    __shared__ uint32_t part[4][3];
    uint32_t c[3] = {0u, 0u, 0u};
    for (int s = static_cast<int>(threadIdx.x); s < n; s += 256) {
        const uint32_t L = lost[s];
        // the stripe's result word is 0 for an empty mask and for lost parity alone without decode_parity
        const uint32_t written = decode_parity ? L : L & ((1u << k) - 1u);
        c[xor_masks_rank(nfrag, hd, L) < 0 ? 2 : written == 0u ? 0 : 1]++;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        for (int o = 32; o; o >>= 1) c[i] += __shfl_xor(c[i], o);
        if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6][i] = c[i];
    }
    __syncthreads();
    if (threadIdx.x < 3) counts[threadIdx.x] = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}

std::atomic<long long> g_xor_decode_masks_launches{0};

// The decode table of (k, m, hd) in device memory: made at the first call that asks, per (device, code),
// and kept for the life of the process (at most 2952 entries of 16 bytes each).  ECAMD_EINVAL for a code
// init_xor_hd_code rejects.
int xor_masks_table(int dev, int k, int m, int hd, const XorMasksEntry** out)
{
    static CodeTables<4> tables("decode table upload");
    const void* d = nullptr;
    const int rc = tables.get({dev, k, m, hd}, [&](std::vector<uint8_t>& bytes) {
        bytes.resize(static_cast<size_t>(kXorMasksMaxEntries) * sizeof(XorMasksEntry));
        const int count = ecamd_xor_decode_masks_plan(k, m, hd, bytes.data(), kXorMasksMaxEntries);
        if (count < 1 || count > kXorMasksMaxEntries) return dev_fail(ECAMD_EINVAL, "no decode table for the flat XOR code (%d,%d,%d)", k, m, hd);
        bytes.resize(static_cast<size_t>(count) * sizeof(XorMasksEntry));
        return 0;
    }, &d);
    *out = static_cast<const XorMasksEntry*>(d);
    return rc;
}

}  // namespace

extern "C" {

int ecamd_xor_decode_masks(int k, int m, int hd, const uint32_t* d_lost, int decode_parity, void* base, int64_t stripe_stride,
                           int64_t frag_stride, int64_t blocksize, int nstripes, uint32_t* d_result, uint32_t* d_counts,
                           void* stream)
{
    int dev = 0;
    int rc = dev_ensure(&dev);
    if (rc) return rc;
    if (k <= 0 || m <= 0 || k + m > 32 || ecamd_xor_code_tables(k, m, hd, nullptr, nullptr) != 0)
        return dev_fail(ECAMD_EINVAL, "(%d,%d,%d) is not a flat_xor_hd code", k, m, hd);
    const StripeLayout lay{static_cast<uint8_t*>(base), stripe_stride, frag_stride, blocksize, nstripes};
    if (!d_lost || !lay.sane()) return dev_fail(ECAMD_EINVAL, "bad masks / base / blocksize / strides");
    if (!lay.aligned16()) return dev_fail(ECAMD_EINVAL, "fragment addresses must be 16-byte aligned");
    if (nstripes == 0) return 0;
    const XorMasksEntry* d_table = nullptr;
    if ((rc = xor_masks_table(dev, k, m, hd, &d_table))) return rc;
    const auto st = static_cast<hipStream_t>(stream);
    XorMasksArgs a{};
    a.base = lay.base;
    a.lost = d_lost;
    a.table = d_table;
    a.result = d_result;
    a.stripe_stride = stripe_stride;
    a.frag_stride = frag_stride;
    a.len = blocksize;
    a.nstripes = nstripes;
    a.k = k;
    a.n = k + m;
    a.hd = hd;
    a.decode_parity = decode_parity ? 1 : 0;
    int cols = 0, slots = 0;  // a tile column per 16 tiles of 4096 bytes (stripe_grid's units: 16-byte chunks)
    stripe_grid((blocksize + 15) >> 4, nstripes, cols, slots);
    hipLaunchKernelGGL(xor_decode_masks_kernel, dim3(static_cast<unsigned>(cols), static_cast<unsigned>(slots)), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    g_xor_decode_masks_launches.fetch_add(1, std::memory_order_relaxed);
    if (d_counts) {
        hipLaunchKernelGGL(xor_masks_counts_kernel, dim3(1), dim3(256), 0, st, d_lost, nstripes, k, k + m, hd,
                           a.decode_parity, d_counts);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

long long ecamd_xor_decode_masks_launches(void) { return g_xor_decode_masks_launches.load(std::memory_order_relaxed); }

}  // extern "C"
