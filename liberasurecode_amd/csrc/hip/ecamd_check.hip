// ecamd_check.hip -- stripe integrity on the device: check, locate, the pair stage, correct, scrub, and the
// same for flat XOR stripes with fragments missing (DESIGN.md "Consistency check", "Locate and scrub",
// "Two bad fragments", "Correct on the device", "Degraded flat XOR stripes", "Check driver: one call record").
//
// d_status[s]: the checked fragments of stripe s that disagree with its inputs.  d_suspects[s] (locate):
// the fragments that ALONE explain every disagreement of stripe s.  d_pairs[s] (pair stage): the two
// fragments that together do.  A correcting call then XORs the error values into the stored words.
//
// The driver.  Every entry point builds one CheckCall -- where the stripes lie (StripeLayout), the stream,
// the result arrays, how far the call goes -- and hands it to its family's builder (rs_call, xor_call,
// xor_degraded_call) through check_entry: device, the family's test of the code, check_layout, the
// CheckPlan, the caller's `checked` / `covered` word, run_check.  run_check lays the plan's fragments out
// as Participants (the K inputs, then the R checked rows) once, and every stage reads that record:
//   fused stage    whole tiles, by the plan's Fused tag.  rs_vand: ecamd::check_fused (ecamd_device.hip), the
//                  check / locate form of the bitsliced kernel over the syndrome map [A | I].  Flat XOR:
//                  xor_check_kernel below, the syndromes straight from 128-bit loads of every fragment, or
//                  (fragments missing) of the participants alone (XorCheckSlotArgs).
//   generic stage  everything else -- tails, small fragments, shapes the fused kernels decline, maps still
//                  compiling, knob bitslice 0, knob xor_check_fused 0: the strided applies compute the
//                  expected fragments into the stream context's scratch (slot kCheckScratchSlot, at most
//                  kCheckScratchBytes, so long batches go stripe chunk by stripe chunk and long fragments
//                  byte range by byte range) and check_compare_kernel / locate_compare_kernel compare.
//   finalize       (locate) locate_finalize_kernel masks the suspects with the participating fragments
//                  and clears them on clean stripes.  Both stages before it OR into the same status
//                  words and AND into the same suspects, which run_check sets first.
//   pair stage     (rs_vand, R >= 4) locate_pairs_kernel reads the dirty stripes without a suspect again
//                  and ORs into d_pairs[s] the fragments its words need; pairs_finalize_kernel keeps a
//                  word of exactly two bits.
//   correct stage  correct_kernel reads the three words of each stripe and XORs the error values of a
//                  located fragment or pair into the stored words.
// All of it on the caller's stream, in order, with no host wait; only the scrubs wait, in scrub_located.
//
// Each section keeps its kernels, their argument structs and the device tables they read together
// (PairsTable / check_map_pairs, CorrectTable / check_map_correct / xor_correct_table; the cached check
// map of ecamd_rs.hip only owns the memory of the first two, OnceTable).  with_groups picks kernel<N> for
// a count of load groups; stripe_grid, the grid of the stripe-by-stripe kernels, is shared with
// ecamd_decode_masks.hip.  The extern "C" block at the end goes by operation: check, locate, pairs,
// correct, degraded, scrub, prebuild, counters.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "../host/gf16.hpp"
#include "../host/tune.hpp"
#include "ecamd.h"
#include "ecamd_host.h"
#include "ecamd_internal.hpp"
#include "ecamd_isa.hpp"

using namespace ecamd;

namespace {

// One call of the driver, built once by its entry point.  suspects is null for a check and pairs for a
// call without a pair stage, so no stage asks again what kind of call it serves.
struct CheckCall {
    StripeLayout lay;
    uint32_t* status;
    void* stream;
    uint32_t* suspects = nullptr;
    uint32_t* pairs = nullptr;
    uint32_t* counts = nullptr;  // of a correcting call; may stay null
    bool locates = false, pairs_asked = false, corrects = false;
    int dev = 0;  // check_entry sets it

    CheckCall(const void* base, int64_t stripe_stride, int64_t frag_stride, int64_t blocksize, int nstripes, uint32_t* d_status,
              void* s)
        : lay{static_cast<uint8_t*>(const_cast<void*>(base)), stripe_stride, frag_stride, blocksize, nstripes},
          status(d_status), stream(s)
    {
    }
    CheckCall& locate(uint32_t* d_suspects) { return locates = true, suspects = d_suspects, *this; }
    CheckCall& pair(uint32_t* d_pairs) { return pairs_asked = true, pairs = d_pairs, *this; }
    CheckCall& correct(uint32_t* d_counts) { return corrects = true, counts = d_counts, *this; }  // writes through lay.base
    hipStream_t st() const { return static_cast<hipStream_t>(stream); }
};

struct CheckCmpArgs {
    const uint8_t* base;  // stored: row r of stripe s at base + s*stripe_stride + off[r]
    const uint8_t* calc;  // computed: row r of stripe s at calc + (s*nrows + r)*pitch
    uint32_t* status;     // of the launch's first stripe
    int64_t stripe_stride;
    int64_t pitch;
    int64_t len;          // bytes compared per fragment
    int64_t off[32];
    uint8_t bit[32];
    int nrows;
};

// grid (x, row, stripe): 16-byte pieces of exactly `len` bytes, the last piece masked to the
// fragment's own bytes (read byte by byte, so nothing past `len` is ever touched); one atomicOr per
// (wave, row) that differs, none for a wave that sees no difference.
__global__ void __launch_bounds__(256) check_compare_kernel(CheckCmpArgs a)
{
    const int r = blockIdx.y;
    const int64_t s = blockIdx.z;
    const uint8_t* x = a.base + s * a.stripe_stride + a.off[r];
    const uint8_t* y = a.calc + (s * a.nrows + r) * a.pitch;
    const int64_t whole = a.len >> 4;
    uint32_t d = 0;
    for (int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; p < whole;
         p += static_cast<int64_t>(gridDim.x) * 256) {
        const uint4 u = *reinterpret_cast<const uint4*>(x + p * 16);
        const uint4 v = *reinterpret_cast<const uint4*>(y + p * 16);
        d |= (u.x ^ v.x) | (u.y ^ v.y) | (u.z ^ v.z) | (u.w ^ v.w);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = whole << 4; i < a.len; i++) d |= static_cast<uint32_t>(x[i] ^ y[i]);
    if (__ballot(d != 0u) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(a.status + s, 1u << a.bit[r]);
}

// Locate, generic stage: the compare step also names the single fragment that explains a stripe's
// disagreements.  The R x K map A (R checked rows over K inputs) comes as rat[r*K + j] =
// A[r][j] / A[piv[j]][j], piv[j] the first row with A[r][j] != 0 and colmask[j] the rows where it is
// non-zero (rs_vand: every row, piv 0; flat XOR: the parity bitmaps, all ratios 1).  R * K <= 256
// because K + R <= 32.
constexpr int kLocMaxRK = 256;
struct LocateCmpArgs {
    const uint8_t* base;  // as CheckCmpArgs
    const uint8_t* calc;
    uint32_t* status;
    uint32_t* suspects;  // of the launch's first stripe
    int64_t stripe_stride;
    int64_t pitch;
    int64_t len;
    int64_t off[32];
    uint32_t colmask[32];
    uint16_t rat[kLocMaxRK];
    uint8_t piv[32];
    uint8_t row_bit[32];  // fragment index of checked row r
    uint8_t in_bit[32];   // fragment index of input j
    int nrows, ncols;
};

// c times both 16-bit words of x in GF(2^16), polynomial 0x1100b: shift and xor, no table.
__device__ __forceinline__ uint32_t gf16_mul2(uint32_t c, uint32_t x)
{
    uint32_t acc = 0;
#pragma unroll
    for (int b = 0; b < 16; b++) {
        if ((c >> b) & 1u) acc ^= x;
        const uint32_t hi = x & 0x80008000u;
        x = ((x & 0x7fff7fffu) << 1) ^ ((hi >> 15) * 0x100bu);
    }
    return acc;
}

// Syndrome piece p (16 bytes) of one row: stored ^ computed; the last, partial piece byte by byte
// and zero-padded, so nothing past `len` is ever read.
__device__ __forceinline__ uint4 locate_piece(const uint8_t* x, const uint8_t* y, int64_t p, int64_t whole, int64_t len)
{
    if (p < whole) {
        const uint4 u = *reinterpret_cast<const uint4*>(x + p * 16);
        const uint4 v = *reinterpret_cast<const uint4*>(y + p * 16);
        return uint4{u.x ^ v.x, u.y ^ v.y, u.z ^ v.z, u.w ^ v.w};
    }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int64_t q = (whole << 4) + i;
        const uint32_t d = q < len ? static_cast<uint32_t>(x[q] ^ y[q]) : 0u;
        w[i >> 2] |= d << (8 * (i & 3));
    }
    return uint4{w[0], w[1], w[2], w[3]};
}

// grid (x, stripe): one thread takes all R rows of a 16-byte piece.  Status bits as
// check_compare_kernel.  For a dirty piece only: checked candidate c survives iff row c alone is
// non-zero; input candidate j survives iff exactly the rows of colmask[j] are non-zero and
// S_r == rat[r][j] * S_piv for each of them.  A dirty wave issues one atomicOr and one atomicAnd.
__global__ void __launch_bounds__(256) locate_compare_kernel(LocateCmpArgs a)
{
    const int64_t s = blockIdx.y;
    const uint8_t* xs = a.base + s * a.stripe_stride;
    const uint8_t* ys = a.calc + s * a.nrows * a.pitch;
    const int64_t whole = a.len >> 4, pieces = (a.len + 15) >> 4;
    uint32_t st = 0u, keep = 0xffffffffu;
    for (int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; p < pieces;
         p += static_cast<int64_t>(gridDim.x) * 256) {
        uint32_t nz = 0u;
        for (int r = 0; r < a.nrows; r++) {
            const uint4 d = locate_piece(xs + a.off[r], ys + r * a.pitch, p, whole, a.len);
            if ((d.x | d.y | d.z | d.w) != 0u) nz |= 1u << r;
        }
        if (nz == 0u) continue;
        for (int r = 0; r < a.nrows; r++) {
            if ((nz >> r) & 1u) st |= 1u << a.row_bit[r];
            if (nz != (1u << r)) keep &= ~(1u << a.row_bit[r]);
        }
        for (int j = 0; j < a.ncols; j++) {
            bool ok = nz == a.colmask[j];
            if (ok) {
                const int pv = a.piv[j];
                const uint4 s0 = locate_piece(xs + a.off[pv], ys + pv * a.pitch, p, whole, a.len);
                for (int r = 0; r < a.nrows && ok; r++) {
                    if (r == pv || !((nz >> r) & 1u)) continue;
                    const uint32_t c = a.rat[r * a.ncols + j];
                    const uint4 d = locate_piece(xs + a.off[r], ys + r * a.pitch, p, whole, a.len);
                    ok = gf16_mul2(c, s0.x) == d.x && gf16_mul2(c, s0.y) == d.y && gf16_mul2(c, s0.z) == d.z &&
                         gf16_mul2(c, s0.w) == d.w;
                }
            }
            if (!ok) keep &= ~(1u << a.in_bit[j]);
        }
    }
    for (int o = 32; o; o >>= 1) {
        st |= __shfl_xor(st, o);
        keep &= __shfl_xor(keep, o);
    }
    if ((threadIdx.x & 63u) == 0u && st != 0u) {
        atomicOr(a.status + s, st);
        atomicAnd(a.suspects + s, keep);
    }
}

// suspects[s] = status[s] ? suspects[s] & participating : 0 (the last step of a locate call); with
// `pairs` (ecamd_rs_locate_pairs) it also sets pairs[s] to 0 for the pair stage that follows.
__global__ void __launch_bounds__(256) locate_finalize_kernel(const uint32_t* status, uint32_t* suspects,
                                                              uint32_t participating, int n, uint32_t* pairs)
{
    const int s = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (s < n) {
        suspects[s] = status[s] ? suspects[s] & participating : 0u;
        if (pairs) pairs[s] = 0u;
    }
}

// ---- rs_vand, two bad fragments: locate_pairs_kernel (ecamd_rs_locate_pairs) -------------------
// Runs after a locate, on its results: a stripe that is dirty and has no suspect is read again, the
// K inputs and the R checked fragments directly (no scratch), 4 bytes -- two words -- per lane at a
// time.  The participants are the K inputs, then the R checked rows; the table (PairsTable) holds what
// tests one of them and what tests a pair.
//
// The pair plan of a cached check map (rs_locate_pairs_plan, host/gf16.hpp) as the device table
// locate_pairs_kernel reads (built by check_map_pairs below).  Entries of 2 + R words: [0] fragment a |
// fragment b << 8 | pivot row p << 16 | pivot row q << 24, [1] the rows a single participant must leave
// non-zero -- exactly those --, [2 + r] L[r][0] | L[r][1] << 16.  First the K + R single participants (b
// and q 0xff; L[r][0] = column[r] / column[p], p its first non-zero row), then the pairs that can be
// tested (dependent ones left out).  `exact`: any four columns of [A | I] are independent, so the pair is
// unique; dev is null when it is not, or when R < 4 (the call then leaves d_pairs zero).  At most 18 KiB.
struct PairsTable {
    const uint32_t* dev = nullptr;
    int singles = 0, pairs = 0, stride = 0;
    bool exact = false;
};
constexpr int kPairsMaxRows = 31;  // K + R <= 32; R >= 4 leaves K <= 28
struct PairsArgs {
    const uint8_t* base;  // participant c of stripe s at base + s*stripe_stride + off[c]
    const uint32_t* status;
    const uint32_t* suspects;
    uint32_t* pairs;
    const uint32_t* table;
    int64_t stripe_stride;
    int64_t len;  // bytes per fragment, even
    int64_t off[32];
    uint32_t cmask[kPairsMaxRows * 16];  // [r*16 + b]: the inputs j whose A[r][j] has bit b
    int32_t nstripes, K, R, singles, npairs, stride;
};

// Unit u (4 bytes) of a fragment; the last, partial unit byte by byte and zero-padded, so nothing
// past `len` is ever read.
__device__ __forceinline__ uint32_t pairs_unit(const uint8_t* x, int64_t u, int64_t whole, int64_t len)
{
    if (u < whole) return *reinterpret_cast<const uint32_t*>(x + u * 4);
    uint32_t w = 0u;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int64_t q = (whole << 2) + i;
        if (q < len) w |= static_cast<uint32_t>(x[q]) << (8 * i);
    }
    return w;
}

// Does the single participant of table entry e explain the lane's unit (syndrome row r at syn[r*256],
// non-zero rows nz)?  Exactly the rows of its column are non-zero and proportional to the pivot row.
__device__ __forceinline__ bool pairs_single_ok(const uint32_t* e, const uint32_t* syn, int R, uint32_t nz)
{
    if (e[1] != nz) return false;
    const int p = static_cast<int>((e[0] >> 16) & 0xffu);
    const uint32_t sp = syn[p * 256];
    for (int r = 0; r < R; r++) {
        if (r == p || !((nz >> r) & 1u)) continue;
        if (gf16_mul2(e[2 + r] & 0xffffu, sp) != syn[r * 256]) return false;
    }
    return true;
}

// Does the pair of table entry e explain it?  S_r == L[r][0]*S_p ^ L[r][1]*S_q for every other row.
__device__ __forceinline__ bool pairs_pair_ok(const uint32_t* e, const uint32_t* syn, int R)
{
    const int p = static_cast<int>((e[0] >> 16) & 0xffu), q = static_cast<int>(e[0] >> 24);
    const uint32_t sp = syn[p * 256], sq = syn[q * 256];
    for (int r = 0; r < R; r++) {
        if (r == p || r == q) continue;
        const uint32_t l = e[2 + r];
        if ((gf16_mul2(l & 0xffffu, sp) ^ gf16_mul2(l >> 16, sq)) != syn[r * 256]) return false;
    }
    return true;
}

__device__ __forceinline__ uint32_t pairs_bits(uint32_t w) { return (1u << (w & 0x1fu)) | (1u << ((w >> 8) & 0x1fu)); }

// grid (chunks, stripe slots), grid-stride over both; K <= 4*KG.  A workgroup loads status[s] and
// suspects[s] and goes on only for a dirty stripe without a suspect: on a clean batch every
// workgroup ends after these two loads per stripe.  Per unit: the K inputs in registers, syndrome
// row r = stored row r ^ sum_j A[r][j] * input j in Horner form over the coefficient bits (XOR the
// inputs whose coefficient has bit b -- wave-uniform masks from the arguments --, double, 16 times),
// the R rows in LDS (row r of lane t at [r*256 + t]; each lane reads only its own).  A dirty unit
// ORs into the lane's mask: 1 << a when single participant a explains it; else both bits of the
// workgroup's hint pair when that explains it; else those of the first pair of the table that does,
// which becomes the hint; else all ones.  One atomicOr per wave with a non-zero mask (relaxed, agent
// scope); pairs_finalize_kernel keeps a word of exactly two bits.  With any four columns of [A | I]
// independent (the table exists only then) the pairs that explain a word are every pair that
// contains one participant, exactly one pair, or none -- so the OR over the dirty units has exactly
// two bits iff one pair explains them all, whichever of a word's pairs the hint made a lane take.
// The hint is reset per stripe, between barriers every lane of the workgroup reaches.
template <int KG>
__global__ void __launch_bounds__(256) locate_pairs_kernel(const PairsArgs a)
{
    extern __shared__ uint32_t pairs_lds[];  // R rows of 256 syndromes, the hint
    uint32_t* syn = pairs_lds + threadIdx.x;
    uint32_t* hint = pairs_lds + a.R * 256;
    const int64_t whole = a.len >> 2, units = (a.len + 3) >> 2;
    for (int s = static_cast<int>(blockIdx.y); s < a.nstripes; s += static_cast<int>(gridDim.y)) {
        if (a.status[s] == 0u || a.suspects[s] != 0u) continue;  // the same for every lane
        if (threadIdx.x == 0) *hint = 0xffffffffu;
        __syncthreads();
        const uint8_t* xs = a.base + static_cast<int64_t>(s) * a.stripe_stride;
        uint32_t mask = 0u;
        for (int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; u < units;
             u += static_cast<int64_t>(gridDim.x) * 256) {
            uint32_t in[4 * KG];
#pragma unroll
            for (int j = 0; j < 4 * KG; j++) in[j] = j < a.K ? pairs_unit(xs + a.off[j], u, whole, a.len) : 0u;
            uint32_t nz = 0u;
            for (int r = 0; r < a.R; r++) {
                uint32_t acc = 0u;
                for (int b = 15; b >= 0; b--) {
                    const uint32_t hi = acc & 0x80008000u;
                    acc = ((acc & 0x7fff7fffu) << 1) ^ ((hi >> 15) * 0x100bu);
                    const uint32_t m = a.cmask[r * 16 + b];
#pragma unroll
                    for (int j = 0; j < 4 * KG; j++) acc = xor_and(acc, in[j], 0u - ((m >> j) & 1u));
                }
                acc ^= pairs_unit(xs + a.off[a.K + r], u, whole, a.len);
                syn[r * 256] = acc;
                if (acc != 0u) nz |= 1u << r;
            }
            if (nz == 0u) continue;
            uint32_t got = 0u;
            for (int c = 0; c < a.singles && got == 0u; c++) {
                const uint32_t* e = a.table + c * a.stride;
                if (pairs_single_ok(e, syn, a.R, nz)) got = 1u << (e[0] & 0x1fu);
            }
            if (got == 0u) {
                const uint32_t h = __hip_atomic_load(hint, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (h != 0xffffffffu) {
                    const uint32_t* e = a.table + h * a.stride;
                    if (pairs_pair_ok(e, syn, a.R)) got = pairs_bits(e[0]);
                }
            }
            for (int i = a.singles; i < a.singles + a.npairs && got == 0u; i++) {
                const uint32_t* e = a.table + i * a.stride;
                if (pairs_pair_ok(e, syn, a.R)) {
                    got = pairs_bits(e[0]);
                    __hip_atomic_store(hint, static_cast<uint32_t>(i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
            mask |= got != 0u ? got : 0xffffffffu;
        }
        for (int o = 32; o; o >>= 1) mask |= __shfl_xor(mask, o);
        if ((threadIdx.x & 63u) == 0u && mask != 0u)
            __hip_atomic_fetch_or(a.pairs + s, mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();  // no lane still stores this stripe's hint when the next one's is reset
    }
}

// pairs[s] = the word when it has exactly two bits, else 0 (the last step of ecamd_rs_locate_pairs).
__global__ void __launch_bounds__(256) pairs_finalize_kernel(uint32_t* pairs, int n)
{
    const int s = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (s < n) {
        const uint32_t v = pairs[s];
        pairs[s] = __popc(v) == 2 ? v : 0u;
    }
}

std::atomic<long long> g_pairs_launches{0};

// PairsArgs / CorrectArgs cmask of the R x K matrix A: [r*16 + b] the inputs j whose A[r][j] has bit b.
void fill_cmask(const std::vector<int>& A, int K, int R, uint32_t* cmask)
{
    for (int r = 0; r < R; r++)
        for (int j = 0; j < K; j++)
            for (int b = 0; b < 16; b++)
                if ((A[static_cast<size_t>(r) * K + j] >> b) & 1) cmask[r * 16 + b] |= 1u << j;
}

// What PairsArgs and CorrectArgs share, and the grid both kernels take (stripe_grid): a chunk per 16
// passes of 256 units -- on a clean batch a launch costs what its empty workgroups cost (11 us for 16384
// of them, traced).
template <class Args>
dim3 located_args(Args& a, const CheckCall& c, const std::vector<int>& A, const Participants& p, const uint32_t* table)
{
    a.base = c.lay.base;
    a.status = c.status;
    a.suspects = c.suspects;
    a.pairs = c.pairs;
    a.table = table;
    a.stripe_stride = c.lay.stripe_stride;
    a.len = c.lay.blocksize;
    std::copy(p.off, p.off + p.K + p.R, a.off);
    fill_cmask(A, p.K, p.R, a.cmask);
    a.nstripes = c.lay.nstripes;
    a.K = p.K;
    int chunks = 0, slots = 0;
    stripe_grid((c.lay.blocksize + 3) >> 2, c.lay.nstripes, chunks, slots);
    return dim3(static_cast<unsigned>(chunks), static_cast<unsigned>(slots));
}

// The pair stage of one call, after locate_finalize_kernel on the same stream, which has set d_pairs
// to 0: with R >= 4 and a table, locate_pairs_kernel and its finalize.
int locate_pairs(const CheckCall& c, const std::vector<int>& A, const Participants& p, const PairsTable& t)
{
    if (p.R < 4 || p.R > kPairsMaxRows || !t.dev || !t.exact) return 0;
    PairsArgs a{};
    const dim3 grid = located_args(a, c, A, p, t.dev), block(256);
    a.R = p.R;
    a.singles = t.singles;
    a.npairs = t.pairs;
    a.stride = t.stride;
    const size_t lds = (static_cast<size_t>(p.R) * 256 + 1) * sizeof(uint32_t);
    with_groups<1, 7>((p.K + 3) / 4, [&](auto g) {  // K <= 28
        hipLaunchKernelGGL(locate_pairs_kernel<decltype(g)::value>, grid, block, lds, c.st(), a);
    });
    HIP_TRY(hipGetLastError());
    g_pairs_launches.fetch_add(1, std::memory_order_relaxed);
    hipLaunchKernelGGL(pairs_finalize_kernel, dim3(static_cast<unsigned>((c.lay.nstripes + 255) / 256)), dim3(256), 0, c.st(),
                       c.pairs, c.lay.nstripes);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- correct on the device: correct_kernel (ecamd_rs_correct, ecamd_xor_correct) ----------------
// Runs after a locate (or the pair stage), on its results and on the same stream: a located error is an
// error VALUE.  With S_r = stored_r ^ sum_j A[r][j] * in_j, the one bad participant c of a stripe has
// e_c = scale[c] * S_pivot[c] in every word, and a located pair {a, b} with pivot rows (p, q) has
// (e_a, e_b) = inv(M) (S_p, S_q), M the 2 x 2 minor the pair plan picked.  XORing the error value into
// the stored word gives the codeword that agrees with every other participant -- the fragment a
// decode would write, byte for byte -- so only the words that are wrong are written.
//
// The correction plan (rs_correct_plan, host/gf16.hpp) as the device table correct_kernel reads.  Words
// [0, 32): for fragment f, participant c | pivot row << 8 | scale << 16, all ones for a fragment that
// takes no part.  With `pairs` (R >= 2), from word 32 three words per pair of participants a < b in the
// pair plan's order: pivot row p | pivot row q << 8 (0xff each for dependent columns), minv[0] | minv[1]
// << 16, minv[2] | minv[3] << 16.  At most 32 + 3 * 496 words.  rs_vand: check_map_correct below, kept
// with the cached check map; flat XOR: the 32 words alone (xor_correct_table).
struct CorrectTable {
    const uint32_t* dev = nullptr;
    bool pairs = false;
};
struct CorrectArgs {
    uint8_t* base;  // participant c of stripe s at base + s*stripe_stride + off[c]
    const uint32_t* status;
    const uint32_t* suspects;
    const uint32_t* pairs;  // null: singles only
    const uint32_t* table;
    int64_t stripe_stride;
    int64_t len;  // bytes per fragment, even
    int64_t off[32];
    uint32_t cmask[kPairsMaxRows * 16];  // as PairsArgs
    int32_t nstripes, K, P;
};

// Syndrome row `row` (wave-uniform) of the lane's unit: Horner over the coefficient bits, as
// locate_pairs_kernel takes it.  A bit no coefficient of the row has (flat XOR: all but bit 0) costs
// the doubling only.
template <int KG>
__device__ __forceinline__ uint32_t correct_syndrome(const CorrectArgs& a, const uint32_t (&in)[4 * KG], int row,
                                                     const uint8_t* xs, int64_t u, int64_t whole)
{
    uint32_t acc = 0u;
    for (int b = 15; b >= 0; b--) {
        const uint32_t hi = acc & 0x80008000u;
        acc = ((acc & 0x7fff7fffu) << 1) ^ ((hi >> 15) * 0x100bu);
        const uint32_t m = a.cmask[row * 16 + b];
        if (m == 0u) continue;
#pragma unroll
        for (int j = 0; j < 4 * KG; j++) acc = xor_and(acc, in[j], 0u - ((m >> j) & 1u));
    }
    return acc ^ pairs_unit(xs + a.off[a.K + row], u, whole, a.len);
}

// XOR the non-zero error value e into unit u of the fragment at x: one 4-byte read and store; the
// last, partial unit byte by byte, so nothing at or past `len` is read or written.
__device__ __forceinline__ void correct_unit(uint8_t* x, int64_t u, int64_t whole, int64_t len, uint32_t e)
{
    if (u < whole) {
        uint32_t* w = reinterpret_cast<uint32_t*>(x + u * 4);
        *w ^= e;
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int64_t q = (whole << 2) + i;
        if (q < len) x[q] ^= static_cast<uint8_t>(e >> (8 * i));
    }
}

// grid (chunks, stripe slots), grid-stride over both, as locate_pairs_kernel; K <= 4*KG.  A workgroup
// loads status[s], suspects[s] and, when given, pairs[s] -- through readfirstlane, so the case and
// everything selected by it (table entry, pivot rows, constants, offsets) are scalar -- and goes on only
// for a stripe with exactly one suspect or, without a suspect, a pair of exactly two bits: a clean
// batch costs those loads and nothing else.  Per unit of such a stripe: the K inputs in registers, the
// one or two pivot rows' syndromes, the error value(s) by gf16_mul2 with the stripe's constants; a
// non-zero error value is XORed into the stored unit of the fragment, a zero one writes nothing.  The
// only unit a lane writes is the one it read, and no other lane reads it: no synchronisation, no LDS.
template <int KG>
__global__ void __launch_bounds__(256) correct_kernel(const CorrectArgs a)
{
    const int64_t whole = a.len >> 2, units = (a.len + 3) >> 2;
    for (int s = static_cast<int>(blockIdx.y); s < a.nstripes; s += static_cast<int>(gridDim.y)) {
        if (__builtin_amdgcn_readfirstlane(a.status[s]) == 0u) continue;
        const uint32_t sus = __builtin_amdgcn_readfirstlane(a.suspects[s]);
        const uint32_t two = sus == 0u && a.pairs ? __builtin_amdgcn_readfirstlane(a.pairs[s]) : 0u;
        const bool single = sus != 0u && (sus & (sus - 1u)) == 0u;
        if (!single && __popc(two) != 2) continue;
        // [f]: participant | pivot row << 8 | scale << 16 of fragment f, all ones when it takes no part
        uint32_t ea = a.table[__builtin_ctz(single ? sus : two)], eb = 0xffffffffu;
        int p = static_cast<int>((ea >> 8) & 0xffu), q = 0;
        uint32_t m01 = ea >> 16, m23 = 0u;  // single: the scale
        if (!single) {
            eb = a.table[31 - __builtin_clz(two)];
            if (ea == 0xffffffffu || eb == 0xffffffffu) continue;
            if ((ea & 0xffu) > (eb & 0xffu)) {
                const uint32_t t = ea;
                ea = eb;
                eb = t;
            }
            // pair i of participants ca < cb at [32 + 3i]: p | q << 8, minv[0] | minv[1] << 16, minv[2] | minv[3] << 16
            const int ca = static_cast<int>(ea & 0xffu), cb = static_cast<int>(eb & 0xffu);
            const uint32_t* e = a.table + 32 + 3 * (ca * (2 * a.P - ca - 1) / 2 + (cb - ca - 1));
            p = static_cast<int>(e[0] & 0xffu);
            q = static_cast<int>((e[0] >> 8) & 0xffu);
            m01 = e[1];
            m23 = e[2];
        }
        if (ea == 0xffffffffu || p == 0xff) continue;  // (never: a located fragment takes part, a located pair is independent)
        uint8_t* xs = a.base + static_cast<int64_t>(s) * a.stripe_stride;
        uint8_t* xa = xs + a.off[ea & 0xffu];
        uint8_t* xb = xs + a.off[eb & 0x1fu];
        for (int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; u < units;
             u += static_cast<int64_t>(gridDim.x) * 256) {
            uint32_t in[4 * KG];
#pragma unroll
            for (int j = 0; j < 4 * KG; j++) in[j] = j < a.K ? pairs_unit(xs + a.off[j], u, whole, a.len) : 0u;
            const uint32_t sp = correct_syndrome<KG>(a, in, p, xs, u, whole);
            if (single) {
                const uint32_t e = gf16_mul2(m01, sp);
                if (e != 0u) correct_unit(xa, u, whole, a.len, e);
            } else {
                const uint32_t sq = correct_syndrome<KG>(a, in, q, xs, u, whole);
                const uint32_t e0 = gf16_mul2(m01 & 0xffffu, sp) ^ gf16_mul2(m01 >> 16, sq);
                const uint32_t e1 = gf16_mul2(m23 & 0xffffu, sp) ^ gf16_mul2(m23 >> 16, sq);
                if (e0 != 0u) correct_unit(xa, u, whole, a.len, e0);
                if (e1 != 0u) correct_unit(xb, u, whole, a.len, e1);
            }
        }
    }
}

// counts[0..3] = stripes clean, with exactly one suspect, with a pair and no suspect, dirty with
// neither -- the cases correct_kernel tells apart.  One workgroup; the four words are overwritten.
__global__ void __launch_bounds__(256) correct_counts_kernel(const uint32_t* status, const uint32_t* suspects,
                                                             const uint32_t* pairs, int n, uint32_t* counts)
{
    __shared__ uint32_t part[4][4];
    uint32_t c[4] = {0u, 0u, 0u, 0u};
    for (int s = static_cast<int>(threadIdx.x); s < n; s += 256) {
        const uint32_t sus = suspects[s];
        if (status[s] == 0u)
            c[0]++;
        else if (sus != 0u && (sus & (sus - 1u)) == 0u)
            c[1]++;
        else if (sus == 0u && pairs && __popc(pairs[s]) == 2)
            c[2]++;
        else
            c[3]++;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        for (int o = 32; o; o >>= 1) c[i] += __shfl_xor(c[i], o);
        if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6][i] = c[i];
    }
    __syncthreads();
    if (threadIdx.x < 4) counts[threadIdx.x] = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}

std::atomic<long long> g_correct_launches{0};

// The correction of one call, after the locate's (or the pair stage's) last kernel on the same
// stream: correct_kernel and, with counts, the counts.  Nothing here waits for the stream or copies
// to the host -- the case of every stripe is decided on the device.  A null: nothing was checked.
int correct_located(const CheckCall& c, const std::vector<int>* A, const Participants& p, const CorrectTable& t)
{
    if (p.R >= 1 && p.R <= kPairsMaxRows && t.dev) {  // no checked fragment: every stripe reads clean
        CorrectArgs a{};
        const dim3 grid = located_args(a, c, *A, p, t.dev), block(256);
        if (!t.pairs) a.pairs = nullptr;
        a.P = p.K + p.R;
        with_groups<1, 8>((p.K + 3) / 4, [&](auto g) {  // K <= 31
            hipLaunchKernelGGL(correct_kernel<decltype(g)::value>, grid, block, 0, c.st(), a);
        });
        HIP_TRY(hipGetLastError());
        g_correct_launches.fetch_add(1, std::memory_order_relaxed);
    }
    if (c.counts) {
        hipLaunchKernelGGL(correct_counts_kernel, dim3(1), dim3(256), 0, c.st(), c.status, c.suspects, c.pairs, c.lay.nstripes,
                           c.counts);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// ---- flat XOR, fused stage: xor_check_kernel -------------------------------------------------
constexpr int kXorCheckMaxFrags = 28;  // 7 load groups of 4; the accepted codes have k + m <= 26
constexpr int kXorCheckMaxRows = 6;    // m of the accepted codes: 3, 5, 6
struct XorCheckArgs {
    const uint8_t* base;  // of the launch's first stripe; fragment f of stripe s at base + s*stripe_stride + off32[f]
    uint32_t* status;     // of the launch's first stripe
    uint32_t* suspects;   // locate form only
    int64_t stripe_stride;
    uint32_t records;  // bytes of a stripe the buffer resource covers: furthest fragment + the covered bytes
    uint32_t tiles_per_stripe;
    int32_t nfrags, nrows, k;
    int32_t off32[kXorCheckMaxFrags];
    uint32_t masks[kXorCheckMaxRows];  // row p: parity bitmap p | 1 << (k + p), the stored parity folded in
    uint32_t sig[kXorCheckMaxFrags];   // ecamd_xor_check_plan
};
// The degraded form (ecamd_xor_check_degraded and its kin): the same fields over SLOTS, the available
// fragments that occur in a surviving row of ecamd_xor_check_plan_degraded, ascending -- nfrags of them,
// off32 / sig per slot, masks over slot numbers, sig over the nrows surviving rows packed densely -- and
// the two tables that turn a slot and a packed row back into result bits.  k is unused.
struct XorCheckSlotArgs : XorCheckArgs {
    uint8_t slot_frag[kXorCheckMaxFrags];  // fragment index of slot i: its suspect bit
    uint8_t row_bit[kXorCheckMaxRows];     // status bit of packed row r: k + the parity that owns it
};

// The check (LOCATE false) and locate form of flat XOR over whole tiles, one workgroup per tile of
// blockDim.x * 16 bytes; grid = tiles_per_stripe * stripes.  The input side of xor_stream_kernel: one
// buffer resource per stripe, all k + m fragments in unconditional groups of four 128-bit loads (the
// unused slots of the last group read zeros through an out-of-range offset), inputs unrolled.
// Syndrome row p accumulates fragment f under the wave-uniform bit f of masks[p] -- the stored parity
// is fragment k + p of its own row, so S_p = stored parity p ^ XOR of the data in bitmap p comes out of
// the same v_bitop3 chain: m <= 6 rows of 4 dwords, no LDS, no scratch.
// Stage 1: one ballot per row; a wave with no non-zero row is done -- no store, no atomic.  The check
// form ORs the rows' bits into the status.  Stage 2 (locate, dirty waves only, from the registers): a
// dirty lane keeps the one fragment f with sig[f] == the lane's set of non-zero rows, provided those
// rows' 16 bytes are equal, else none.  That is the per-word rule of ecamd_xor_check_plan ANDed over
// the lane's 8 words: a clean word has no non-zero row, so "every dirty word has rows sig[f], all
// equal" is "the 16-byte rows of sig[f] are equal and every other row is zero".  keep is ANDed across
// the wave; one lane issues one atomicOr and one atomicAnd (relaxed, agent scope), as
// locate_compare_kernel ends.
// With Args = XorCheckSlotArgs this is the degraded form: the same tile over the slots, so KG comes from
// the participant count -- a lost fragment, and an available one that no surviving row contains, is
// never loaded -- and a row's status bit and a slot's suspect bit come from the two tables.
template <int KG, bool LOCATE, class Args>
__global__ void __launch_bounds__(256) xor_check_kernel(const Args a)
{
    constexpr bool SLOTS = std::is_same_v<Args, XorCheckSlotArgs>;
    typedef unsigned int v4 __attribute__((ext_vector_type(4)));
    const uint32_t t = blockIdx.x;
    const uint32_t s = t / a.tiles_per_stripe;
    const int off = static_cast<int>((t - s * a.tiles_per_stripe) * (blockDim.x * 16u) + threadIdx.x * 16u);
    const auto rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.base) + static_cast<int64_t>(s) * a.stripe_stride,
                                                       0, static_cast<int>(a.records), 0x00020000);
    v4 syn[kXorCheckMaxRows];
#pragma unroll
    for (int r = 0; r < kXorCheckMaxRows; r++) syn[r] = v4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int g = 0; g < KG; g++) {
        v4 x[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int f = 4 * g + i;
            const int o = (f < a.nfrags) ? a.off32[f] + off : static_cast<int>(0x80000000u);
            x[i] = __builtin_amdgcn_raw_buffer_load_b128(rin, o, 0, 2);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int f = 4 * g + i;
#pragma unroll
            for (int r = 0; r < kXorCheckMaxRows; r++) {
                if (r >= a.nrows) break;
                const uint32_t msk = 0u - ((a.masks[r] >> f) & 1u);  // wave-uniform
#pragma unroll
                for (int d = 0; d < 4; d++) syn[r][d] = xor_and(syn[r][d], x[i][d], msk);
            }
        }
    }
    uint32_t nz = 0u, bits = 0u;  // this lane's non-zero rows; the wave's, as status bits
#pragma unroll
    for (int r = 0; r < kXorCheckMaxRows; r++) {
        if (r >= a.nrows) break;
        const bool dirty = (syn[r][0] | syn[r][1] | syn[r][2] | syn[r][3]) != 0u;
        if (dirty) nz |= 1u << r;
        if constexpr (SLOTS) {
            if (__ballot(dirty) != 0ull) bits |= 1u << a.row_bit[r];
        } else {
            if (__ballot(dirty) != 0ull) bits |= 1u << (a.k + r);
        }
    }
    if (bits == 0u) return;
    if constexpr (!LOCATE) {
        if ((threadIdx.x & 63u) == 0u) __hip_atomic_fetch_or(a.status + s, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        uint32_t keep = 0xffffffffu;
        if (nz != 0u) {
            v4 first = v4{0u, 0u, 0u, 0u};
            bool have = false, equal = true;
#pragma unroll
            for (int r = 0; r < kXorCheckMaxRows; r++) {
                if (!((nz >> r) & 1u)) continue;
                if (!have) {
                    first = syn[r];
                    have = true;
                } else if (((syn[r][0] ^ first[0]) | (syn[r][1] ^ first[1]) | (syn[r][2] ^ first[2]) | (syn[r][3] ^ first[3])) != 0u) {
                    equal = false;
                }
            }
            keep = 0u;
            if (equal)
                for (int f = 0; f < a.nfrags; f++)
                    if (a.sig[f] == nz) {
                        if constexpr (SLOTS)
                            keep |= 1u << a.slot_frag[f];
                        else
                            keep |= 1u << f;
                    }
        }
        for (int o = 32; o; o >>= 1) keep &= __shfl_xor(keep, o);
        if ((threadIdx.x & 63u) == 0u) {
            __hip_atomic_fetch_or(a.status + s, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_and(a.suspects + s, keep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

std::atomic<long long> g_xor_check_fused{0}, g_xor_locate_fused{0};

// The slots of a degraded flat XOR plan (ecamd_xor_check_plan_degraded), what the degraded form of
// xor_check_kernel works on: the participants -- the available fragments that occur in a surviving row,
// ascending -- and the surviving rows packed densely in the order of their owners, the checked fragments.
struct XorSlots {
    std::vector<int> frag;        // fragment index of slot i
    std::vector<uint32_t> masks;  // packed row r over slot numbers
    std::vector<uint32_t> sig;    // slot i over packed rows
};

// What the entry points differ in: who takes part, the map between them, and which kernel takes the
// whole tiles.  Made in place by its family's builder and not copied (A may point into it).
enum class Fused { kNone, kRsBitsliced, kXorFull, kXorSlots };
struct CheckPlan {
    Fused fused = Fused::kNone;
    int K = 0, R = 0;
    uint8_t frag[32] = {};                // fragment index of input j at [j], of checked row r at [K + r]
    const std::vector<int>* A = nullptr;  // R x K over GF(2^16): checked row r = sum of A[r][j] * input j (null: R == 0)
    // rs_vand: the cached check map, what A points into; its map computes the checked rows in the generic stage
    CheckMap cached;
    // flat XOR: the rows over the inputs as 0 / 1, what A points to; the generic stage takes them as masks
    std::vector<int> bitmaps;
    std::vector<uint32_t> sig;  // kXorFull: the signatures of ecamd_xor_check_plan
    XorSlots slots;             // kXorSlots
    PairsTable pairs;           // ecamd_rs_locate_pairs
    CorrectTable correct;       // a correcting call
    CheckPlan() = default;
    CheckPlan(const CheckPlan&) = delete;
    CheckPlan& operator=(const CheckPlan&) = delete;
    void input(int f) { frag[K++] = static_cast<uint8_t>(f); }  // all of them before the first checked row
    void checked(int f) { frag[K + R++] = static_cast<uint8_t>(f); }
};

// Row r of the 0 / 1 matrix A (R x K) as a mask over its K inputs.
uint32_t row_mask(const std::vector<int>& A, int K, int r)
{
    uint32_t v = 0;
    for (int j = 0; j < K; j++) v |= static_cast<uint32_t>(A[static_cast<size_t>(r) * K + j] & 1) << j;
    return v;
}

// Fused stage of a flat XOR check or, with suspects, locate over the whole tiles of every fragment.
// Geometry as launch_xor: one-wave workgroups on 1 KiB tiles or 256-lane workgroups on 4 KiB tiles
// (knob xor_check_threads 64 / 256), one workgroup per tile, long batches as launches of
// xor_tiles_per_slot tiles (of 4 KiB) per slot with xor_wgs (0: 3) slots per CU.  By default one-wave
// tiles at every size, where launch_xor takes them from 256 KiB: on clean data they tie with 4 KiB tiles
// at (10,6,4) x 1 MiB (0.614 against 0.615 ms) and win every repetition at (3,3,3) x 4 KiB (0.473
// against 0.486 ms; tools/check_bench.py --xor, profiles/xor_check.json).  Returns
// the bytes of each fragment covered, or 0 with nothing launched when it declines: knob
// xor_check_fused 0, a fragment shorter than a tile, a stripe the 32-bit buffer offsets cannot span.
// xor_check_tiles is the part both argument forms share: `a` comes with its tables filled, `last` is the
// highest fragment index it loads.  Load groups -- full stripes: 2 ((3,3,3): 6 fragments) to 7 ((20,6,4):
// 26); degraded: 1 (up to 4 participants) to 7.
template <class Args>
int64_t xor_check_tiles(const CheckCall& c, Args& a, int last)
{
    constexpr bool kSlots = std::is_same_v<Args, XorCheckSlotArgs>;
    const StripeLayout& l = c.lay;
    if (!g_tune.xor_check_fused || l.nstripes <= 0) return 0;
    const int knob_threads = g_tune.xor_check_threads;
    const int threads = knob_threads ? knob_threads : 64;
    const int64_t tile = static_cast<int64_t>(threads) * 16;
    const int64_t cover = l.blocksize / tile * tile;
    if (cover == 0 || l.stripe_stride < 0) return 0;
    if (last * l.frag_stride + l.blocksize >= (int64_t(1) << 31)) return 0;
    const uint64_t tps = static_cast<uint64_t>(cover / tile);
    const int wgs_knob = g_tune.xor_wgs;
    const int wgs = wgs_knob > 0 ? wgs_knob : 3;
    const uint64_t slots = static_cast<uint64_t>(dev_cu_count(c.dev)) * static_cast<uint64_t>(wgs);
    const uint64_t limit = static_cast<uint64_t>(std::max<int>(g_tune.xor_tiles_per_slot, 0)) * static_cast<uint64_t>(256 / threads);
    const int per = launch_stripes(l.nstripes, tps, slots, limit);
    if (tps * static_cast<uint64_t>(per) > 0x7fffffffull) return 0;
    a.stripe_stride = l.stripe_stride;
    a.records = static_cast<uint32_t>(last * l.frag_stride + cover);
    a.tiles_per_stripe = static_cast<uint32_t>(tps);
    for (int i = 0; i < a.nfrags; i++) {
        int f = i;
        if constexpr (kSlots) f = a.slot_frag[i];
        a.off32[i] = static_cast<int32_t>(f * l.frag_stride);
    }
    const bool locate = c.suspects != nullptr;
    for (int s0 = 0; s0 < l.nstripes; s0 += per) {
        const int ns = std::min(per, l.nstripes - s0);
        a.base = l.base + s0 * l.stripe_stride;
        a.status = c.status + s0;
        a.suspects = locate ? c.suspects + s0 : nullptr;
        const dim3 grid(static_cast<unsigned>(tps * static_cast<uint64_t>(ns))), block(static_cast<unsigned>(threads));
        with_groups<kSlots ? 1 : 2, 7>((a.nfrags + 3) / 4, [&](auto g) {
            if (locate)
                hipLaunchKernelGGL((xor_check_kernel<decltype(g)::value, true, Args>), grid, block, 0, c.st(), a);
            else
                hipLaunchKernelGGL((xor_check_kernel<decltype(g)::value, false, Args>), grid, block, 0, c.st(), a);
        });
        HIP_TRY(hipGetLastError());
        (locate ? g_xor_locate_fused : g_xor_check_fused).fetch_add(1, std::memory_order_relaxed);
    }
    return cover;
}

// Full stripes: fragment f of the k + m at f*frag_stride, row r the parity bitmap with the stored parity
// folded in.
int64_t xor_check_fused(const CheckCall& c, const CheckPlan& p)
{
    const int k = p.K, m = p.R, n = k + m;
    if (n <= 4 || n > kXorCheckMaxFrags || m > kXorCheckMaxRows) return 0;
    XorCheckArgs a{};
    a.nfrags = n;
    a.nrows = m;
    a.k = k;
    for (int f = 0; f < n; f++) a.sig[f] = p.sig[static_cast<size_t>(f)];
    for (int r = 0; r < m; r++) a.masks[r] = row_mask(*p.A, k, r) | (1u << (k + r));
    return xor_check_tiles(c, a, n - 1);
}

// The same stage for a degraded stripe: only the participants are loaded, in (participants + 3) / 4
// groups.  Declines as xor_check_fused does, and for a plan without a surviving row.
int64_t xor_check_fused_slots(const CheckCall& c, const CheckPlan& p)
{
    const XorSlots& sl = p.slots;
    const int n = static_cast<int>(sl.frag.size()), rows = p.R;
    if (n < 1 || n > kXorCheckMaxFrags || rows < 1 || rows > kXorCheckMaxRows) return 0;
    XorCheckSlotArgs a{};
    a.nfrags = n;
    a.nrows = rows;
    for (int i = 0; i < n; i++) {
        a.sig[i] = sl.sig[static_cast<size_t>(i)];
        a.slot_frag[i] = static_cast<uint8_t>(sl.frag[static_cast<size_t>(i)]);
    }
    for (int r = 0; r < rows; r++) {
        a.masks[r] = sl.masks[static_cast<size_t>(r)];
        a.row_bit[r] = p.frag[p.K + r];
    }
    return xor_check_tiles(c, a, sl.frag.back());
}

// Generic stage: bytes [from, blocksize) of the checked rows of every stripe against what the plan's
// apply computes from the inputs.  `from` a multiple of 16.  With `loc` (its map tables, input bits
// and suspects filled in) the compare step is locate_compare_kernel, which writes the status bits too.
int check_generic(const CheckCall& c, const CheckPlan& p, const Participants& pt, int64_t from, const LocateCmpArgs* loc)
{
    const StripeLayout& l = c.lay;
    const int nrows = pt.R, nstripes = l.nstripes;
    const int64_t bs = l.blocksize;
    if (from >= bs || nrows <= 0 || nstripes <= 0) return 0;
    std::vector<uint32_t> masks;  // flat XOR: ecamd_xor_apply_strided over the rows of A
    if (!p.cached.map)
        for (int r = 0; r < nrows; r++) masks.push_back(row_mask(*p.A, pt.K, r));
    const int64_t cap = static_cast<int64_t>(kCheckScratchBytes);
    const int64_t seg = std::max<int64_t>(65536, cap / nrows / 65536 * 65536);  // fragment bytes per pass
    for (int64_t f0 = from; f0 < bs; f0 += seg) {
        const int64_t len = std::min(seg, bs - f0);
        const int64_t pitch = (len + 255) & ~int64_t(255);
        const int per = static_cast<int>(std::min<int64_t>(std::clamp<int64_t>(cap / (pitch * nrows), 1, 65535), nstripes));
        uint32_t* scratch = nullptr;
        int rc = stream_scratch(c.dev, c.stream, kCheckScratchSlot, static_cast<size_t>(per) * nrows * pitch / 4, &scratch);
        if (rc) return rc;
        auto* calc = reinterpret_cast<uint8_t*>(scratch);
        std::vector<int64_t> io(pt.off, pt.off + pt.K), oo;
        for (auto& v : io) v += f0;
        for (int r = 0; r < nrows; r++) oo.push_back(r * pitch);
        for (int s0 = 0; s0 < nstripes; s0 += per) {
            const int ns = std::min(per, nstripes - s0);
            const uint8_t* in = l.base + s0 * l.stripe_stride;
            rc = p.cached.map ? ecamd_map_apply_strided(p.cached.map, in, l.stripe_stride, io.data(), calc, nrows * pitch, oo.data(),
                                                        len, ns, c.stream)
                              : ecamd_xor_apply_strided(masks.data(), nrows, pt.K, in, l.stripe_stride, io.data(), calc,
                                                        nrows * pitch, oo.data(), len, ns, c.stream);
            if (rc) return rc;
            // the fields both compare kernels take
            auto common = [&](auto& a, uint8_t* row_bit) {
                a.base = in + f0;
                a.calc = calc;
                a.status = c.status + s0;
                a.stripe_stride = l.stripe_stride;
                a.pitch = pitch;
                a.len = len;
                a.nrows = nrows;
                std::copy(pt.off + pt.K, pt.off + pt.K + nrows, a.off);
                std::copy(pt.bit + pt.K, pt.bit + pt.K + nrows, row_bit);
            };
            if (loc) {
                LocateCmpArgs la = *loc;
                common(la, la.row_bit);
                la.suspects = loc->suspects + s0;
                const unsigned lx = static_cast<unsigned>(std::clamp<int64_t>((((len + 15) >> 4) + 1023) / 1024, 1, 1024));
                hipLaunchKernelGGL(locate_compare_kernel, dim3(lx, static_cast<unsigned>(ns)), dim3(256), 0, c.st(), la);
            } else {
                CheckCmpArgs ca{};
                common(ca, ca.bit);
                const unsigned gx = static_cast<unsigned>(std::clamp<int64_t>(((len >> 4) + 1023) / 1024, 1, 1024));
                hipLaunchKernelGGL(check_compare_kernel, dim3(gx, static_cast<unsigned>(nrows), static_cast<unsigned>(ns)),
                                   dim3(256), 0, c.st(), ca);
            }
            HIP_TRY(hipGetLastError());
        }
    }
    return 0;
}

// The layout checks of every entry point, a locate's own two, and the pair stage's.
int check_layout(const CheckCall& c)
{
    if (!c.lay.sane() || !c.status) return dev_fail(ECAMD_EINVAL, "bad base / status / blocksize / strides");
    if (!c.lay.aligned16()) return dev_fail(ECAMD_EINVAL, "fragment addresses must be 16-byte aligned");
    if (c.locates && !c.suspects) return dev_fail(ECAMD_EINVAL, "null suspects");
    // an odd size ends in half a word, whose product is cut to 8 bits: proportionality cannot be tested
    if (c.locates && (c.lay.blocksize & 1))
        return dev_fail(ECAMD_EINVAL, "locate needs an even blocksize (%lld)", static_cast<long long>(c.lay.blocksize));
    if (c.pairs_asked && !c.pairs) return dev_fail(ECAMD_EINVAL, "null pairs");
    return 0;
}

// The map tables of LocateCmpArgs for the R x K matrix A (row-major; entries 0..0xffff).  The ratio
// matrix is also computed by rs_locate_map (host planning) and bitslice_locate_ratio (the generated
// kernel); this one stays apart because it alone takes a column's FIRST NON-ZERO row as the pivot and
// masks the rows where the column is zero -- the flat XOR bitmaps have zeros, an rs_vand map has none.
void locate_tables(const std::vector<int>& A, int R, int K, LocateCmpArgs& l)
{
    const GF16& gf = GF16::get();
    l.nrows = R;
    l.ncols = K;
    for (int j = 0; j < K; j++) {
        int pv = -1;
        uint32_t mask = 0;
        for (int r = 0; r < R; r++)
            if (A[static_cast<size_t>(r) * K + j]) {
                if (pv < 0) pv = r;
                mask |= 1u << r;
            }
        l.piv[j] = static_cast<uint8_t>(std::max(pv, 0));
        l.colmask[j] = mask;
        for (int r = 0; r < R; r++)
            l.rat[r * K + j] = pv < 0 ? 0 : static_cast<uint16_t>(gf.mul(A[static_cast<size_t>(r) * K + j],
                                                                         gf.inv(A[static_cast<size_t>(pv) * K + j])));
    }
}

// One validated call: both arrays set, the fused stage over whole tiles, the generic stage over the
// rest, the finalize step of a locate, the pair stage on its results and the correction on both.
// StreamUse: the scratch of the stream context outlives the call.
int run_check(const CheckCall& c, const CheckPlan& p)
{
    const StripeLayout& l = c.lay;
    if (l.nstripes == 0) return 0;
    const StreamUse use(c.dev, c.stream);
    const size_t words = static_cast<size_t>(l.nstripes) * sizeof(uint32_t);
    if (c.suspects) HIP_TRY(hipMemsetAsync(c.suspects, 0xff, words, c.st()));
    HIP_TRY(hipMemsetAsync(c.status, 0, words, c.st()));
    const int K = p.K, R = p.R;
    Participants pt;
    pt.K = K;
    pt.R = R;
    for (int i = 0; i < K + R; i++) {
        pt.bit[i] = p.frag[i];
        pt.off[i] = p.frag[i] * l.frag_stride;
        pt.mask |= 1u << p.frag[i];
    }
    // fewer than 2 checked fragments tell nothing apart: the two stages run as a check, then the finalize
    // names every participating fragment of a dirty stripe
    CheckCall stage = c;
    if (R < 2) stage.suspects = nullptr;
    const bool locating = stage.suspects != nullptr;
    // whole tiles through the fused kernel; what it covered is done, the rest of each fragment goes
    // the generic way
    int64_t cover = 0;
    switch (p.fused) {
    case Fused::kRsBitsliced:
        if (locating) {
            // one launch over all R rows: the second stage needs every row's syndrome in one wave, so
            // more than 8 rows are declined and take the generic stage alone
            cover = check_fused(c.dev, *p.A, pt, 0, R, l, c.status, c.suspects, c.stream);
        } else {
            // one launch per group of 8 rows; only what EVERY group covered is done
            cover = l.blocksize;
            for (int row0 = 0; row0 < R && cover >= 0; row0 += 8)
                cover = std::min(cover, check_fused(c.dev, *p.A, pt, row0, std::min(8, R - row0), l, c.status, nullptr, c.stream));
        }
        break;
    case Fused::kXorFull:  // one launch reads all K + R fragments of a tile and takes the syndromes from the loads
        cover = xor_check_fused(stage, p);
        break;
    case Fused::kXorSlots:  // the same over the participants of the reduced rows alone
        cover = xor_check_fused_slots(stage, p);
        break;
    case Fused::kNone: break;
    }
    if (cover < 0) return static_cast<int>(cover);
    LocateCmpArgs loc{};
    if (locating) {
        loc.suspects = c.suspects;
        locate_tables(*p.A, R, K, loc);
        std::copy(pt.bit, pt.bit + K, loc.in_bit);
    }
    const int rc = check_generic(stage, p, pt, cover, locating ? &loc : nullptr);
    if (rc || !c.suspects) return rc;
    hipLaunchKernelGGL(locate_finalize_kernel, dim3(static_cast<unsigned>((l.nstripes + 255) / 256)), dim3(256), 0, c.st(),
                       c.status, c.suspects, pt.mask, l.nstripes, c.pairs);
    HIP_TRY(hipGetLastError());
    if (c.pairs && R >= 4) {  // fewer than four checks leave d_pairs zero
        const int prc = locate_pairs(c, *p.A, pt, p.pairs);
        if (prc) return prc;
    }
    return c.corrects ? correct_located(c, p.A, pt, p.correct) : 0;
}

// The pair table of a cached check map (PairsTable above), made at the first call that asks for it and
// kept with the map (cm.pairs: freed with the entry, not counted against the map cache's byte limit).
int check_map_pairs(const CheckMap& cm, PairsTable& out)
{
    out = PairsTable();
    OnceTable* t = cm.pairs;
    if (!t || !cm.coeff) return 0;
    const std::vector<int>&inputs = *cm.inputs, &outputs = *cm.checked;
    const int K = static_cast<int>(inputs.size()), R = static_cast<int>(outputs.size());
    std::call_once(t->once, [&] {
        const PairPlan plan = rs_locate_pairs_plan(*cm.coeff, R, K);
        if (!plan.pairs || !plan.independent4) return;  // no table: d_pairs stays zero
        const GF16& gf = GF16::get();
        const int P = K + R;
        auto frag = [&](int c) { return static_cast<uint32_t>(c < K ? inputs[c] : outputs[c - K]); };
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
        int i = 0;
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
            }
        const void* d = nullptr;
        if ((t->rc = upload_table("pair table", tab.data(), tab.size() * sizeof(uint32_t), &d))) return;
        t->dev = static_cast<const uint32_t*>(d);
        t->words = tab.size();
    });
    if (t->rc) return dev_fail(ECAMD_EHIP, "pair table upload failed");
    if (!t->dev) return 0;
    out.dev = t->dev;
    out.singles = K + R;
    out.stride = 2 + R;
    out.pairs = static_cast<int>(t->words) / out.stride - out.singles;  // the entries after the singles
    out.exact = true;
    return 0;
}

// The correction table of a cached check map (CorrectTable above), the same way (cm.correct).
int check_map_correct(const CheckMap& cm, CorrectTable& out)
{
    out = CorrectTable();
    OnceTable* t = cm.correct;
    if (!t || !cm.coeff) return 0;  // nothing checked: nothing to correct
    std::call_once(t->once, [&] {
        const std::vector<int>&inputs = *cm.inputs, &outputs = *cm.checked;
        const int K = static_cast<int>(inputs.size()), R = static_cast<int>(outputs.size());
        const CorrectPlan plan = rs_correct_plan(*cm.coeff, R, K);
        const int P = K + R;
        if (P > 32 || static_cast<int>(plan.pivot.size()) != P) return;
        std::vector<uint32_t> tab(32, 0xffffffffu);
        for (int c = 0; c < P; c++) {
            const int f = c < K ? inputs[c] : outputs[c - K];
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
        const void* d = nullptr;
        if ((t->rc = upload_table("correction table", tab.data(), tab.size() * sizeof(uint32_t), &d))) return;
        t->dev = static_cast<const uint32_t*>(d);
        t->words = tab.size();
    });
    if (t->rc) return dev_fail(ECAMD_EHIP, "correction table upload failed");
    out.dev = t->dev;
    out.pairs = t->words > 32;
    return 0;
}

// The correction table of a flat XOR code (CorrectTable above) from its check plan:
// fragment f is participant f, its pivot the lowest row of sig[f], every scale 1.  Device memory made
// at the first call that asks, per (device, k, m, hd, mask of lost fragments), and kept for the life of
// the process (a few accepted codes and the loss patterns a caller meets, 128 bytes each).  With
// fragments lost (a kXorSlots plan) fragment f is the participant correct_kernel loads in its place --
// its index among the plan's inputs, or K + r for the owner of packed row r -- and its pivot the packed
// row of the lowest bit of sig[f]; a fragment no surviving row contains takes no part.
int xor_correct_table(int dev, int k, int m, int hd, uint32_t lost, const unsigned* sig, const CheckPlan& plan, CorrectTable& out)
{
    static CodeTables<5> tables("correction table");
    const void* d = nullptr;
    const int rc = tables.get({dev, k, m, hd, static_cast<int>(lost)}, [&](std::vector<uint8_t>& bytes) {
        uint32_t tab[32];
        for (int f = 0; f < 32; f++)
            tab[f] = f < k + m && sig[f] ? static_cast<uint32_t>(f) | static_cast<uint32_t>(__builtin_ctz(sig[f])) << 8 | 1u << 16
                                         : 0xffffffffu;
        if (plan.fused == Fused::kXorSlots) {
            const uint8_t* inputs = plan.frag;
            const uint8_t* checked = plan.frag + plan.K;
            for (int f = 0; f < k + m; f++) {
                if (tab[f] == 0xffffffffu) continue;
                int part = -1, row = -1;
                for (int j = 0; j < plan.K; j++)
                    if (inputs[j] == f) part = j;
                for (int r = 0; r < plan.R; r++) {
                    if (checked[r] == f) part = plan.K + r;
                    if (row < 0 && checked[r] == k + __builtin_ctz(sig[f])) row = r;
                }
                tab[f] = part < 0 || row < 0 ? 0xffffffffu : static_cast<uint32_t>(part) | static_cast<uint32_t>(row) << 8 | 1u << 16;
            }
        }
        bytes.resize(sizeof(tab));
        std::memcpy(bytes.data(), tab, sizeof(tab));
        return 0;
    }, &d);
    out.dev = static_cast<const uint32_t*>(d);
    out.pairs = false;
    return rc;
}

// What every entry point runs, in this order: the device, the family's own test of the code (valid), the
// layout, the family's plan (build, which also names the fragments the call covers), the caller's word
// of those -- for an empty batch too --, the stages.
template <class Valid, class Build>
int check_entry(CheckCall c, uint32_t* covered, Valid&& valid, Build&& build)
{
    int rc = dev_ensure(&c.dev);
    if (rc || (rc = valid()) || (rc = check_layout(c))) return rc;
    CheckPlan p;
    uint32_t mask = 0;
    if ((rc = build(c, p, mask))) return rc;
    if (covered) *covered = mask;
    return run_check(c, p);
}

// rs_vand: the cached check map with the tables the call's stages ask for.  A bad layout is reported
// before too many missing fragments: check_entry checks it before the plan is made.
int rs_call(int k, int m, const int* missing, uint32_t* checked, const CheckCall& call)
{
    auto valid = [&] {
        if (k <= 0 || m < 0 || k + m > 32)
            return dev_fail(ECAMD_EINVAL, "%s needs k + m <= 32 (k=%d m=%d)", call.locates ? "locate" : "check", k, m);
        return 0;
    };
    return check_entry(call, checked, valid, [&](const CheckCall& c, CheckPlan& p, uint32_t& mask) {
        int rc = check_map(k, m, missing, p.cached);
        if (rc) return rc;
        if (c.pairs_asked && (rc = check_map_pairs(p.cached, p.pairs))) return rc;
        if (c.corrects && (rc = check_map_correct(p.cached, p.correct))) return rc;
        for (int f : *p.cached.inputs) p.input(f);
        for (int f : *p.cached.checked) {
            p.checked(f);
            mask |= 1u << f;
        }
        p.A = p.cached.coeff;
        p.fused = p.cached.map ? Fused::kRsBitsliced : Fused::kNone;
        return 0;
    });
}

// Flat XOR, full stripes: the parity bitmaps as a 0 / 1 map over GF(2^16).
int xor_call(int k, int m, int hd, const CheckCall& call)
{
    unsigned pb[32], db[32];
    auto valid = [&] {
        if (k <= 0 || m <= 0 || k + m > 32 || ecamd_xor_code_tables(k, m, hd, pb, db) != 0)
            return dev_fail(ECAMD_EINVAL, "not a flat_xor_hd code: k=%d m=%d hd=%d", k, m, hd);
        return 0;
    };
    return check_entry(call, nullptr, valid, [&](const CheckCall& c, CheckPlan& p, uint32_t&) {
        p.sig.resize(static_cast<size_t>(k + m));
        if (ecamd_xor_check_plan(k, m, hd, p.sig.data()) != 0) return dev_fail(ECAMD_EINVAL, "no check plan: k=%d m=%d hd=%d", k, m, hd);
        for (int j = 0; j < k; j++) p.input(j);
        for (int r = 0; r < m; r++) {
            p.checked(k + r);
            for (int j = 0; j < k; j++) p.bitmaps.push_back((pb[r] >> j) & 1u);
        }
        p.A = &p.bitmaps;
        p.fused = Fused::kXorFull;
        return c.corrects ? xor_correct_table(c.dev, k, m, hd, 0u, p.sig.data(), p, p.correct) : 0;
    });
}

// Flat XOR with fragments missing: the rows of ecamd_xor_check_plan_degraded as a check plan.  The owner
// parity of each surviving row is checked, every other participant -- the parities of retired pivot rows
// among them -- is an input, and the map is the reduced rows over those inputs; a fragment that is lost,
// or that no surviving row contains, is in neither list, so no stage reads or writes its slot.  The plan
// is validated before the layout.
int xor_degraded_call(int k, int m, int hd, const int* missing, uint32_t* covered, const CheckCall& call)
{
    unsigned rows[32], sig[32], cov = 0;
    auto valid = [&] {
        if (k <= 0 || m <= 0 || k + m > 32 || ecamd_xor_check_plan_degraded(k, m, hd, missing, rows, sig, &cov) < 0)
            return dev_fail(ECAMD_EINVAL, "not a flat_xor_hd code (k=%d m=%d hd=%d) or a bad list of missing fragments", k, m, hd);
        return 0;
    };
    return check_entry(call, covered, valid, [&](const CheckCall& c, CheckPlan& p, uint32_t& mask) {
        uint32_t lost = 0;
        if (missing)
            for (int i = 0; missing[i] > -1; i++) lost |= 1u << missing[i];
        XorSlots& sl = p.slots;
        for (int f = 0; f < k + m; f++) {
            if (!sig[f]) continue;
            sl.frag.push_back(f);
            if (!(f >= k && rows[f - k])) p.input(f);
        }
        for (int r = 0; r < m; r++)
            if (rows[r]) p.checked(k + r);
        const uint8_t* checked = p.frag + p.K;
        for (int r = 0; r < p.R; r++) {
            const unsigned row = rows[checked[r] - k];
            for (int j = 0; j < p.K; j++) p.bitmaps.push_back(static_cast<int>((row >> p.frag[j]) & 1u));
            uint32_t over_slots = 0;
            for (size_t i = 0; i < sl.frag.size(); i++) over_slots |= ((row >> sl.frag[i]) & 1u) << i;
            sl.masks.push_back(over_slots);
        }
        for (int f : sl.frag) {
            uint32_t packed = 0;  // sig[f], over the owners, over the surviving rows in their packed order
            for (int r = 0; r < p.R; r++) packed |= ((sig[f] >> (checked[r] - k)) & 1u) << r;
            sl.sig.push_back(packed);
        }
        p.A = &p.bitmaps;
        p.fused = Fused::kXorSlots;
        mask = cov;
        return c.corrects && p.R > 0 ? xor_correct_table(c.dev, k, m, hd, lost, sig, p, p.correct) : 0;
    });
}

// The host half of ecamd_rs_scrub, ecamd_xor_scrub and ecamd_rs_scrub_pairs, after the locate: a wait
// for the stream, the arrays read back, the counts, and -- when a stripe has exactly one suspect --
// decode(lists) with lists[2*s..] = {f, -1} for such a stripe and {-1, -1} (the empty list) for every
// other.  After a pair stage the lists are 3 long: {f, -1, -1}, {a, b, -1} for a stripe with a pair, and
// the empty list.
struct ScrubCounts {
    int *clean, *repaired, *repaired_pairs, *unlocated;  // the caller's; any may be null
};
template <class Decode>
int scrub_located(const CheckCall& c, const ScrubCounts& out, Decode&& decode)
{
    const int nstripes = c.lay.nstripes;
    int clean = 0, repaired = 0, unlocated = 0, repaired_pairs = 0;
    const size_t width = c.pairs ? 3 : 2;
    if (nstripes > 0) {
        HIP_TRY(hipStreamSynchronize(c.st()));
        std::vector<uint32_t> status(static_cast<size_t>(nstripes)), suspects(static_cast<size_t>(nstripes));
        HIP_TRY(hipMemcpy(status.data(), c.status, status.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(suspects.data(), c.suspects, suspects.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        std::vector<uint32_t> pairs;
        if (c.pairs) {
            pairs.resize(static_cast<size_t>(nstripes));
            HIP_TRY(hipMemcpy(pairs.data(), c.pairs, pairs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
        std::vector<int> lists(static_cast<size_t>(nstripes) * width, -1);
        for (int s = 0; s < nstripes; s++) {
            const uint32_t sus = suspects[static_cast<size_t>(s)];
            const uint32_t pr = c.pairs ? pairs[static_cast<size_t>(s)] : 0u;
            if (!status[static_cast<size_t>(s)])
                clean++;
            else if (sus && !(sus & (sus - 1))) {
                lists[static_cast<size_t>(s) * width] = __builtin_ctz(sus);
                repaired++;
            } else if (!sus && __builtin_popcount(pr) == 2) {
                lists[static_cast<size_t>(s) * width] = __builtin_ctz(pr);
                lists[static_cast<size_t>(s) * width + 1] = 31 - __builtin_clz(pr);
                repaired_pairs++;
            } else
                unlocated++;
        }
        if (repaired || repaired_pairs) {
            const int rc = decode(lists.data(), static_cast<int>(width));
            if (rc) return rc;
        }
    }
    if (out.clean) *out.clean = clean;
    if (out.repaired) *out.repaired = repaired;
    if (out.unlocated) *out.unlocated = unlocated;
    if (out.repaired_pairs) *out.repaired_pairs = repaired_pairs;
    return 0;
}

// The check map of (k, m, missing) planned on the host alone (build time: no device).
int prebuild_plan(const char* what, int k, int m, const int* missing, const char* arch, const char* dir, FragmentMap& fm)
{
    if (!arch || !dir) return dev_fail(ECAMD_EINVAL, "null arch / dir");
    if (k <= 0 || m < 0 || k + m > 32) return dev_fail(ECAMD_EINVAL, "%s needs k + m <= 32 (k=%d m=%d)", what, k, m);
    return rs_vand_plan(4, k, m, missing, -1, 0, fm);
}

}  // namespace

namespace ecamd {

void stripe_grid(int64_t units, int nstripes, int& chunks, int& slots)
{
    chunks = static_cast<int>(std::clamp<int64_t>((units + 4095) / 4096, 1, 64));
    slots = std::min(nstripes, 4096 / chunks);
    const int cap = g_tune.pairs_grid;
    if (cap > 0) {
        chunks = std::min(chunks, cap);
        slots = std::min(slots, cap);
    }
}

}  // namespace ecamd

extern "C" {

// ---- check ----
int ecamd_rs_check(int k, int m, const int* missing, const void* base, int64_t stripe_stride, int64_t frag_stride,
                   int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* checked, void* stream)
{
    return rs_call(k, m, missing, checked, CheckCall(base, stripe_stride, frag_stride, blocksize, nstripes, d_status, stream));
}

int ecamd_xor_check(int k, int m, int hd, const void* base, int64_t stripe_stride, int64_t frag_stride,
                    int64_t blocksize, int nstripes, uint32_t* d_status, void* stream)
{
    return xor_call(k, m, hd, CheckCall(base, stripe_stride, frag_stride, blocksize, nstripes, d_status, stream));
}

// ---- locate ----
int ecamd_rs_locate(int k, int m, const int* missing, const void* base, int64_t stripe_stride, int64_t frag_stride,
                    int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* d_suspects, uint32_t* checked,
                    void* stream)
{
    return rs_call(k, m, missing, checked,
                   CheckCall(base, stripe_stride, frag_stride, blocksize, nstripes, d_status, stream).locate(d_suspects));
}

int ecamd_xor_locate(int k, int m, int hd, const void* base, int64_t stripe_stride, int64_t frag_stride,
                     int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* d_suspects, void* stream)
{
    return xor_call(k, m, hd, CheckCall(base, stripe_stride, frag_stride, blocksize, nstripes, d_status, stream).locate(d_suspects));
}

// ---- pairs ----
int ecamd_rs_locate_pairs(int k, int m, const int* missing, const void* base, int64_t stripe_stride, int64_t frag_stride,
                          int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* d_suspects, uint32_t* d_pairs,
                          uint32_t* checked, void* stream)
{
    return rs_call(k, m, missing, checked,
                   CheckCall(base, stripe_stride, frag_stride, blocksize, nstripes, d_status, stream).locate(d_suspects).pair(d_pairs));
}

// ---- correct ----
// Locate, then correct in place on the same stream: no wait for the stream, no copy to the host, no
// launch that depends on what the locate found -- correct_kernel reads the per-stripe words itself.
int ecamd_rs_correct(int k, int m, const int* missing, void* base, int64_t stripe_stride, int64_t frag_stride,
                     int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* d_suspects, uint32_t* d_pairs,
                     uint32_t* d_counts, uint32_t* checked, void* stream)
{
    CheckCall c(base, stripe_stride, frag_stride, blocksize, nstripes, d_status, stream);
    c.locate(d_suspects).correct(d_counts);
    if (d_pairs) c.pair(d_pairs);  // without them: single fragments only
    return rs_call(k, m, missing, checked, c);
}

int ecamd_xor_correct(int k, int m, int hd, void* base, int64_t stripe_stride, int64_t frag_stride, int64_t blocksize,
                      int nstripes, uint32_t* d_status, uint32_t* d_suspects, uint32_t* d_counts, void* stream)
{
    return xor_call(k, m, hd,
                    CheckCall(base, stripe_stride, frag_stride, blocksize, nstripes, d_status, stream).locate(d_suspects).correct(d_counts));
}

// ---- degraded: flat XOR with fragments missing ----
int ecamd_xor_check_degraded(int k, int m, int hd, const int* missing, const void* base, int64_t stripe_stride,
                             int64_t frag_stride, int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* covered,
                             void* stream)
{
    return xor_degraded_call(k, m, hd, missing, covered,
                             CheckCall(base, stripe_stride, frag_stride, blocksize, nstripes, d_status, stream));
}

int ecamd_xor_locate_degraded(int k, int m, int hd, const int* missing, const void* base, int64_t stripe_stride,
                              int64_t frag_stride, int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* d_suspects,
                              uint32_t* covered, void* stream)
{
    return xor_degraded_call(k, m, hd, missing, covered,
                             CheckCall(base, stripe_stride, frag_stride, blocksize, nstripes, d_status, stream).locate(d_suspects));
}

int ecamd_xor_correct_degraded(int k, int m, int hd, const int* missing, void* base, int64_t stripe_stride,
                               int64_t frag_stride, int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* d_suspects,
                               uint32_t* d_counts, uint32_t* covered, void* stream)
{
    return xor_degraded_call(
        k, m, hd, missing, covered,
        CheckCall(base, stripe_stride, frag_stride, blocksize, nstripes, d_status, stream).locate(d_suspects).correct(d_counts));
}

// ---- scrub: a locate, a host wait, a decode of what it named ----
int ecamd_rs_scrub(int k, int m, void* base, int64_t stripe_stride, int64_t frag_stride, int64_t blocksize,
                   int nstripes, uint32_t* d_status, uint32_t* d_suspects, int* n_clean, int* n_repaired,
                   int* n_unlocated, void* stream)
{
    if (m < 2) return dev_fail(ECAMD_EINVAL, "scrub needs m >= 2 to tell fragments apart (m=%d)", m);
    const CheckCall c = CheckCall(base, stripe_stride, frag_stride, blocksize, nstripes, d_status, stream).locate(d_suspects);
    if (const int rc = rs_call(k, m, nullptr, nullptr, c)) return rc;
    return scrub_located(c, {n_clean, n_repaired, nullptr, n_unlocated}, [&](const int* lists, int width) {
        return ecamd_rs_decode_multi(k, m, lists, width, 1, base, stripe_stride, frag_stride, blocksize, nstripes, stream);
    });
}

int ecamd_rs_scrub_pairs(int k, int m, void* base, int64_t stripe_stride, int64_t frag_stride, int64_t blocksize,
                         int nstripes, uint32_t* d_status, uint32_t* d_suspects, uint32_t* d_pairs, int* n_clean,
                         int* n_repaired, int* n_repaired_pairs, int* n_unlocated, void* stream)
{
    if (m < 4) return dev_fail(ECAMD_EINVAL, "a pair repair needs m >= 4 (m=%d)", m);
    const CheckCall c =
        CheckCall(base, stripe_stride, frag_stride, blocksize, nstripes, d_status, stream).locate(d_suspects).pair(d_pairs);
    if (const int rc = rs_call(k, m, nullptr, nullptr, c)) return rc;
    return scrub_located(c, {n_clean, n_repaired, n_repaired_pairs, n_unlocated}, [&](const int* lists, int width) {
        return ecamd_rs_decode_multi(k, m, lists, width, 1, base, stripe_stride, frag_stride, blocksize, nstripes, stream);
    });
}

int ecamd_xor_scrub(int k, int m, int hd, void* base, int64_t stripe_stride, int64_t frag_stride, int64_t blocksize,
                    int nstripes, uint32_t* d_status, uint32_t* d_suspects, int* n_clean, int* n_repaired,
                    int* n_unlocated, void* stream)
{
    const CheckCall c = CheckCall(base, stripe_stride, frag_stride, blocksize, nstripes, d_status, stream).locate(d_suspects);
    if (const int rc = xor_call(k, m, hd, c)) return rc;
    return scrub_located(c, {n_clean, n_repaired, nullptr, n_unlocated}, [&](const int* lists, int width) {
        return ecamd_xor_decode_multi(k, m, hd, lists, width, 1, base, stripe_stride, frag_stride, blocksize, nstripes, stream);
    });
}

// ---- prebuild (build time, no GPU): the code objects the fused rs_vand stage will ask for ----
int ecamd_check_prebuild(int k, int m, const int* missing, const char* arch, const char* dir)
{
    FragmentMap fm;
    const int rc = prebuild_plan("check", k, m, missing, arch, dir, fm);
    if (rc) return rc;
    const int R = static_cast<int>(fm.outputs.size()), K = static_cast<int>(fm.inputs.size());
    int built = 0;
    for (int row0 = 0; row0 < R; row0 += 8) {  // as run_check groups them
        const int nrows = std::min(8, R - row0);
        const int r = check_fused_prebuild(fm.coeff, K, row0, nrows, false, arch, dir);
        if (r < 0) return dev_fail(ECAMD_EHIP, "check prebuild failed (%d) for a %dx%d map", r, nrows, K + nrows);
        built += r;
    }
    return built;
}

int ecamd_locate_prebuild(int k, int m, const int* missing, const char* arch, const char* dir)
{
    FragmentMap fm;
    const int rc = prebuild_plan("locate", k, m, missing, arch, dir, fm);
    if (rc) return rc;
    const int R = static_cast<int>(fm.outputs.size()), K = static_cast<int>(fm.inputs.size());
    if (R < 2) return 0;  // as run_check: the check's objects serve
    const int r = check_fused_prebuild(fm.coeff, K, 0, R, true, arch, dir);
    if (r == -6) return 0;  // every build needs scratch: the run time declines the fused form as well
    if (r < 0) return dev_fail(ECAMD_EHIP, "locate prebuild failed (%d) for a %dx%d map", r, R, K + R);
    return r;
}

// ---- counters: launches enqueued by this process ----
long long ecamd_xor_check_fused_launches(void) { return g_xor_check_fused.load(std::memory_order_relaxed); }
long long ecamd_xor_locate_fused_launches(void) { return g_xor_locate_fused.load(std::memory_order_relaxed); }
long long ecamd_locate_pairs_launches(void) { return g_pairs_launches.load(std::memory_order_relaxed); }
long long ecamd_correct_launches(void) { return g_correct_launches.load(std::memory_order_relaxed); }

}  // extern "C"
