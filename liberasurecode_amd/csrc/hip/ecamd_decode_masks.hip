// ecamd_decode_masks.hip -- ecamd_rs_decode_masks and ecamd_frame_status_masks (DESIGN.md "Decode from
// device masks"): rebuild the lost fragments of a batch in which every stripe lost a different set,
// the sets given as one mask word per stripe in DEVICE memory.
//
// Three launches on the caller's stream, whatever the masks hold -- no host wait, no map, no compile:
//   masks_plan_kernel    one wave per stripe: masks_plan (ecamd_masks_plan.hpp) from the code's generator
//                        and d_lost[s] into the stripe's MasksRecord in the stream context's scratch
//                        (slot kMasksPlanScratchSlot), and d_result[s];
//   decode_masks_kernel  grid (tiles, stripe slots), grid-stride over both: a workgroup loads its stripe's
//                        record, skips a stripe with no outputs, builds the stripe's nibble tables in LDS
//                        and streams the stripe's tiles;
//   masks_counts_kernel  with d_counts: the three counts from the records.
// T, the data kernel's tile, is 4096 bytes: 256 lanes of one 16-byte chunk per fragment.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "../host/gf16.hpp"
#include "ecamd.h"
#include "ecamd_internal.hpp"
#include "ecamd_masks_plan.hpp"
#include "ecamd_stream.hpp"

using namespace ecamd;

namespace {

constexpr int kPlanLanes = 64;

// One wave per stripe: the 64 lanes share the elements of each step of masks_plan (the rows of the
// Gauss-Jordan elimination, the n_out x k coefficients), its scratch in LDS, the record straight to
// global memory.  The mask is made scalar, so every branch of the plan is.  Nothing here comes from the
// host but G.
__global__ void __launch_bounds__(kPlanLanes) masks_plan_kernel(const uint16_t* G, int k, int m, const uint32_t* lost,
                                                                int rebuild_parity, MasksRecord* recs, uint32_t* result)
{
    __shared__ MasksPlanWork work;
    const uint32_t s = blockIdx.x;
    const uint32_t L = __builtin_amdgcn_readfirstlane(lost[s]);
    const uint32_t r = masks_plan(G, k, m, L, rebuild_parity, recs + s, &work, static_cast<int>(threadIdx.x), kPlanLanes,
                                  [] { __syncthreads(); });
    if (result && threadIdx.x == 0) result[s] = r;
}

struct MasksArgs {
    uint8_t* base;  // fragment f of stripe s at base + s*stripe_stride + f*frag_stride
    const MasksRecord* recs;
    int64_t stripe_stride, frag_stride;
    int64_t len;  // bytes per fragment, even
    int32_t nstripes, k;
};

// Chunk p (16 bytes) of the fragment at x: one 128-bit load; the last, partial chunk (rem bytes) byte by
// byte and zero-padded, so nothing at or past `len` is read.
__device__ __forceinline__ v4u masks_load(const uint8_t* x, int64_t p, int64_t whole, int rem)
{
    if (p < whole) return __builtin_nontemporal_load(reinterpret_cast<const v4u*>(x + p * 16));
    const uint4 t = load_tail(x + p * 16, rem);
    return v4u{t.x, t.y, t.z, t.w};
}

__device__ __forceinline__ void masks_store(uint8_t* y, int64_t p, int64_t whole, int rem, v4u v)
{
    if (p < whole)
        __builtin_nontemporal_store(v, reinterpret_cast<v4u*>(y + p * 16));
    else
        store_tail(y + p * 16, make_uint4(v[0], v[1], v[2], v[3]), rem);
}

// The lane's chunk of inputs 4G..4G+3.  inw[G]: the fragment indices of the group, one per byte, scalar.
template <int G, int KG>
__device__ __forceinline__ void masks_load_group(const MasksArgs& a, const uint8_t* xs, const uint32_t (&inw)[KG], int64_t p,
                                                 int64_t whole, int rem, v4u (&x)[4])
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        x[i] = v4u{0u, 0u, 0u, 0u};
        if (4 * G + i < a.k)
            x[i] = masks_load(xs + static_cast<int64_t>((inw[G] >> (8 * i)) & 0xffu) * a.frag_stride, p, whole, rem);
    }
}

// Group G's lookups (mac_chunk_nib_imm: the table of input J at a compile-time LDS offset), the loads of
// group G + 1 issued before them so that they are in flight meanwhile, as stream_group does.
template <int W, int G, int KG>
__device__ __forceinline__ void masks_group(const MasksArgs& a, const uint8_t* lds, const uint8_t* xs, const uint32_t (&inw)[KG],
                                            int64_t p, int64_t whole, int rem, const v4u (&x)[4], uint32_t (&acc)[8][W / 2])
{
    v4u nxt[4];
    if constexpr (G + 1 < KG) masks_load_group<G + 1, KG>(a, xs, inw, p, whole, rem, nxt);
    if (4 * G + 0 < a.k) mac_chunk_nib_imm<W, 4 * G + 0>(lds, x[0], acc);
    if (4 * G + 1 < a.k) mac_chunk_nib_imm<W, 4 * G + 1>(lds, x[1], acc);
    if (4 * G + 2 < a.k) mac_chunk_nib_imm<W, 4 * G + 2>(lds, x[2], acc);
    if (4 * G + 3 < a.k) mac_chunk_nib_imm<W, 4 * G + 3>(lds, x[3], acc);
    if constexpr (G + 1 < KG) masks_group<W, G + 1, KG>(a, lds, xs, inw, p, whole, rem, nxt, acc);
}

// grid (tiles, stripe slots), grid-stride over both, as correct_kernel; k <= 4*KG, at most W outputs
// per stripe (W from m, not from the masks).  Per stripe a workgroup
//   - loads the record's counts and index bytes through readfirstlane, so everything selected by them
//     (offsets, row predicates) is scalar, and goes on only for a stripe with outputs: a stripe with
//     nothing lost, or an unrecoverable one, costs that one load;
//   - builds the stripe's nibble tables in LDS (host/tables.cpp build_nibble_tables' image: input j,
//     nibble q, value v at ((j*4 + q)*16 + v) * 2W bytes, row r's product in bytes 2r, 2r+1): an entry is
//     (v << 4q) times two rows' coefficients at once, shift and xor -- the XOR of the c * 2^b of the set
//     bits b.  Rows from n_out up are zero and never stored;
//   - streams the stripe's tiles: 128-bit loads of the k inputs, 32 lookups per input, 128-bit stores of
//     the n_out outputs.  The lost slots are written and never read; nothing else is written.
// The two barriers per stripe are reached by every lane: the record is the same for all of them.
template <int W, int KG>
__global__ void __launch_bounds__(256) decode_masks_kernel(const MasksArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t masks_lds[];
    constexpr int D = W / 2;
    constexpr int EB = 2 * W;
    const int64_t whole = a.len >> 4, chunks = (a.len + 15) >> 4;
    const int rem = static_cast<int>(a.len & 15);
    for (int s = static_cast<int>(blockIdx.y); s < a.nstripes; s += static_cast<int>(gridDim.y)) {
        const MasksRecord* rec = a.recs + s;
        const int n_out = min(static_cast<int>(__builtin_amdgcn_readfirstlane(rec->n_out)), W);
        if (n_out <= 0) continue;
        uint32_t inw[KG], outw[2];
#pragma unroll
        for (int g = 0; g < KG; g++) inw[g] = __builtin_amdgcn_readfirstlane(reinterpret_cast<const uint32_t*>(rec->in)[g]);
#pragma unroll
        for (int g = 0; g < 2; g++) outw[g] = __builtin_amdgcn_readfirstlane(reinterpret_cast<const uint32_t*>(rec->out)[g]);
        __syncthreads();  // the lookups of the previous stripe are over
        for (int e = static_cast<int>(threadIdx.x); e < a.k * 64; e += 256) {
            const int j = e >> 6;
            const uint32_t x = static_cast<uint32_t>(e & 15) << (4 * ((e >> 4) & 3));
            uint32_t* ent = reinterpret_cast<uint32_t*>(masks_lds + e * EB);
#pragma unroll
            for (int d = 0; d < D; d++) {
                const uint32_t c0 = 2 * d < n_out ? rec->coef[(2 * d) * a.k + j] : 0u;
                const uint32_t c1 = 2 * d + 1 < n_out ? rec->coef[(2 * d + 1) * a.k + j] : 0u;
                ent[d] = masks_gf_mul2(x, c0 | (c1 << 16));
            }
        }
        __syncthreads();
        uint8_t* xs = a.base + static_cast<int64_t>(s) * a.stripe_stride;
        for (int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; p < chunks;
             p += static_cast<int64_t>(gridDim.x) * 256) {
            uint32_t acc[8][D];
#pragma unroll
            for (int w = 0; w < 8; w++)
#pragma unroll
                for (int d = 0; d < D; d++) acc[w][d] = 0u;
            v4u first[4];
            masks_load_group<0, KG>(a, xs, inw, p, whole, rem, first);
            masks_group<W, 0, KG>(a, masks_lds, xs, inw, p, whole, rem, first, acc);
#pragma unroll
            for (int r = 0; r < W; r++) {
                if (r >= n_out) break;
                v4u v;
#pragma unroll
                for (int d = 0; d < 4; d++) {
                    const uint32_t A = acc[2 * d][r >> 1], B = acc[2 * d + 1][r >> 1];
                    v[d] = (r & 1) ? ((A >> 16) | (B & 0xffff0000u)) : ((A & 0xffffu) | (B << 16));
                }
                const uint32_t f = (outw[r >> 2] >> (8 * (r & 3))) & 0xffu;
                masks_store(xs + static_cast<int64_t>(f) * a.frag_stride, p, whole, rem, v);
            }
        }
    }
}

// counts[0..2] = stripes left alone (result 0), rebuilt, unrecoverable.  One workgroup; the three
// words are overwritten.
__global__ void __launch_bounds__(256) masks_counts_kernel(const MasksRecord* recs, int n, uint32_t* counts)
{
    __shared__ uint32_t part[4][3];
    uint32_t c[3] = {0u, 0u, 0u};
    for (int s = static_cast<int>(threadIdx.x); s < n; s += 256) {
        const uint32_t r = recs[s].result;
        c[r == 0u ? 0 : (r >> 31) ? 2 : 1]++;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        for (int o = 32; o; o >>= 1) c[i] += __shfl_xor(c[i], o);
        if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6][i] = c[i];
    }
    __syncthreads();
    if (threadIdx.x < 3) counts[threadIdx.x] = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}

// masks[s] = the fragments f of stripe s with status[s*nfrag + f] & bits.
__global__ void __launch_bounds__(256) frame_status_masks_kernel(const uint32_t* status, int nfrag, uint32_t bits, int n,
                                                                 uint32_t* masks)
{
    const int s = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (s >= n) return;
    uint32_t v = 0u;
    for (int f = 0; f < nfrag; f++)
        if (status[static_cast<int64_t>(s) * nfrag + f] & bits) v |= 1u << f;
    masks[s] = v;
}

std::atomic<long long> g_decode_masks_launches{0};

// The generator of (k, m) as 16-bit words in device memory: made at the first call that asks, per
// (device, k, m), and kept for the life of the process (at most 1536 bytes each).
int masks_generator(int dev, int k, int m, const uint16_t** out)
{
    static CodeTables<3> gens("generator upload");
    const void* d = nullptr;
    const int rc = gens.get({dev, k, m}, [&](std::vector<uint8_t>& bytes) {
        const std::vector<int> G = rs_generator(k, m);
        if (G.empty()) return dev_fail(ECAMD_EINVAL, "no generator for k=%d m=%d", k, m);
        const std::vector<uint16_t> g16(G.begin(), G.end());
        bytes.resize(g16.size() * sizeof(uint16_t));
        std::memcpy(bytes.data(), g16.data(), bytes.size());
        return 0;
    }, &d);
    *out = static_cast<const uint16_t*>(d);
    return rc;
}

}  // namespace

extern "C" {

int ecamd_rs_decode_masks(int k, int m, const uint32_t* d_lost, int rebuild_parity, void* base, int64_t stripe_stride,
                          int64_t frag_stride, int64_t blocksize, int nstripes, uint32_t* d_result, uint32_t* d_counts,
                          void* stream)
{
    int dev = 0;
    int rc = dev_ensure(&dev);
    if (rc) return rc;
    if (k <= 0 || m < 0 || k + m > kMasksMaxFrags || m > kMasksMaxOut)
        return dev_fail(ECAMD_EINVAL, "decode_masks needs k + m <= 32 and m <= 8 (k=%d m=%d)", k, m);
    const StripeLayout lay{static_cast<uint8_t*>(base), stripe_stride, frag_stride, blocksize, nstripes};
    if (!d_lost || !lay.sane()) return dev_fail(ECAMD_EINVAL, "bad masks / base / blocksize / strides");
    if (!lay.aligned16()) return dev_fail(ECAMD_EINVAL, "fragment addresses must be 16-byte aligned");
    // an odd size ends in half a word; ecamd_rs_locate and ecamd_rs_correct refuse it as well
    if (blocksize & 1) return dev_fail(ECAMD_EINVAL, "decode_masks needs an even blocksize (%lld)", static_cast<long long>(blocksize));
    if (nstripes == 0) return 0;
    const uint16_t* d_G = nullptr;
    if ((rc = masks_generator(dev, k, m, &d_G))) return rc;
    const StreamUse use(dev, stream);
    const auto st = static_cast<hipStream_t>(stream);
    uint32_t* scratch = nullptr;
    if ((rc = stream_scratch(dev, stream, kMasksPlanScratchSlot, static_cast<size_t>(nstripes) * (sizeof(MasksRecord) / 4), &scratch)))
        return rc;
    auto* recs = reinterpret_cast<MasksRecord*>(scratch);
    hipLaunchKernelGGL(masks_plan_kernel, dim3(static_cast<unsigned>(nstripes)), dim3(kPlanLanes), 0, st, d_G, k, m, d_lost,
                       rebuild_parity ? 1 : 0, recs, d_result);
    HIP_TRY(hipGetLastError());
    MasksArgs a{};
    a.base = lay.base;
    a.recs = recs;
    a.stripe_stride = stripe_stride;
    a.frag_stride = frag_stride;
    a.len = blocksize;
    a.nstripes = nstripes;
    a.k = k;
    int cols = 0, slots = 0;  // a tile column per 16 tiles of 4096 bytes (stripe_grid's units: 16-byte chunks)
    stripe_grid((blocksize + 15) >> 4, nstripes, cols, slots);
    const dim3 grid(static_cast<unsigned>(cols), static_cast<unsigned>(slots));
    const int W = m <= 2 ? 2 : m <= 4 ? 4 : 8;
    const size_t lds = static_cast<size_t>(k) * 64 * 2 * W;
    auto launch = [&](auto w) {
        with_groups<1, 8>((k + 3) / 4, [&](auto g) {  // k <= 32
            hipLaunchKernelGGL((decode_masks_kernel<decltype(w)::value, decltype(g)::value>), grid, dim3(256), lds, st, a);
        });
    };
    if (W == 2)
        launch(std::integral_constant<int, 2>{});
    else if (W == 4)
        launch(std::integral_constant<int, 4>{});
    else
        launch(std::integral_constant<int, 8>{});
    HIP_TRY(hipGetLastError());
    g_decode_masks_launches.fetch_add(1, std::memory_order_relaxed);
    if (d_counts) {
        hipLaunchKernelGGL(masks_counts_kernel, dim3(1), dim3(256), 0, st, recs, nstripes, d_counts);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

long long ecamd_decode_masks_launches(void) { return g_decode_masks_launches.load(std::memory_order_relaxed); }

int ecamd_frame_status_masks(int nfrag, const uint32_t* d_frag_status, uint32_t bits, int nstripes, uint32_t* d_masks,
                             void* stream)
{
    int dev = 0;
    const int rc = dev_ensure(&dev);
    if (rc) return rc;
    if (nfrag < 1 || nfrag > 32 || !d_frag_status || !d_masks || nstripes < 0)
        return dev_fail(ECAMD_EINVAL, "bad status_masks arguments (nfrag=%d)", nfrag);
    if (nstripes == 0) return 0;
    hipLaunchKernelGGL(frame_status_masks_kernel, dim3(static_cast<unsigned>((nstripes + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), d_frag_status, nfrag, bits, nstripes, d_masks);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
