// ecamd_check.hip -- stripe consistency check, locate and scrub (ecamd_rs_check / ecamd_xor_check,
// ecamd_rs_locate / ecamd_xor_locate, ecamd_rs_scrub / ecamd_xor_scrub; DESIGN.md "Consistency check",
// "Locate and scrub").
//
// d_status[s]: the checked fragments of stripe s that disagree with its inputs.  d_suspects[s]
// (locate): the fragments that ALONE explain every disagreement of stripe s.
//
// Fused stage (rs_vand, whole bitsliced tiles; ecamd::check_fused in ecamd_device.hip): the check
// form of the bitsliced kernel over the syndrome map [A | I] reads the K inputs and the R checked
// fragments and writes only the status bits of inconsistent stripes; its locate form also ANDs the
// candidates it rules out away from the suspects.  Fused stage (flat XOR, whole 4 KiB or 1 KiB tiles;
// xor_check_kernel below): the syndromes straight from 128-bit loads of all k + m fragments, the same
// two forms.  Generic stage (everything else: tails, small fragments, shapes the fused kernels
// decline, maps still compiling, knob bitslice 0, knob xor_check_fused 0):
// the strided applies compute the expected fragments into the stream context's scratch (slot
// kCheckScratchSlot, at most kCheckScratchBytes, so long batches go stripe chunk by stripe chunk and
// long fragments byte range by byte range) and check_compare_kernel / locate_compare_kernel compare
// them with the stored ones.  Both stages OR into the same status words and AND into the same
// suspects, which run_check sets first; locate_finalize_kernel masks the suspects with the
// participating fragments and clears them on clean stripes -- all on the caller's stream, in order.
//
// Pair stage (ecamd_rs_locate_pairs, ecamd_rs_scrub_pairs; rs_vand with R >= 4 checked fragments):
// after the finalize, locate_pairs_kernel reads the dirty stripes that have no suspect again and ORs
// into d_pairs[s] the fragments its words need; pairs_finalize_kernel keeps a word of exactly two
// bits (DESIGN.md "Two bad fragments").
//
// Correct stage (ecamd_rs_correct, ecamd_xor_correct): after the locate or the pair stage,
// correct_kernel reads the three words of each stripe and XORs the error values of a located fragment
// or pair into the stored words -- on the same stream, with no host wait (DESIGN.md "Correct on the
// device").  The device tables of the pair and correct stages are laid out and built here, beside the
// kernels that read them (PairsTable / check_map_pairs, CorrectTable / check_map_correct /
// xor_correct_table); the cached check map of ecamd_rs.hip only owns the memory of its two (OnceTable).
// stripe_grid, the grid of the stripe-by-stripe kernels, is shared with ecamd_decode_masks.hip.
//
// Flat XOR with fragments missing (ecamd_xor_check_degraded, ecamd_xor_locate_degraded,
// ecamd_xor_correct_degraded): the rows of ecamd_xor_check_plan_degraded through the same stages -- the
// fused kernel over the participants alone (XorCheckSlotArgs), the generic stage and correct_kernel over
// a CheckPlan of the reduced rows (DESIGN.md "Degraded flat XOR stripes").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
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

// The pair stage of one call, after locate_finalize_kernel on the same stream, which has set d_pairs
// to 0: with R >= 4 and a table, locate_pairs_kernel and its finalize.  The grid (stripe_grid): a chunk
// per 16 passes of 256 units -- on a clean batch the launch costs what its empty workgroups cost (11 us
// for 16384 of them, traced).
int locate_pairs(const std::vector<int>& A, int K, int R, const PairsTable& t, const uint8_t* base, int64_t stripe_stride,
                 const int64_t* in_off, const int64_t* chk_off, int64_t blocksize, int nstripes, const uint32_t* d_status,
                 const uint32_t* d_suspects, uint32_t* d_pairs, hipStream_t st)
{
    if (R < 4 || R > kPairsMaxRows || !t.dev || !t.exact) return 0;
    PairsArgs a{};
    a.base = base;
    a.status = d_status;
    a.suspects = d_suspects;
    a.pairs = d_pairs;
    a.table = t.dev;
    a.stripe_stride = stripe_stride;
    a.len = blocksize;
    for (int j = 0; j < K; j++) a.off[j] = in_off[j];
    for (int r = 0; r < R; r++) a.off[K + r] = chk_off[r];
    fill_cmask(A, K, R, a.cmask);
    a.nstripes = nstripes;
    a.K = K;
    a.R = R;
    a.singles = t.singles;
    a.npairs = t.pairs;
    a.stride = t.stride;
    int chunks = 0, slots = 0;
    stripe_grid((blocksize + 3) >> 2, nstripes, chunks, slots);
    const dim3 grid(static_cast<unsigned>(chunks), static_cast<unsigned>(slots)), block(256);
    const size_t lds = (static_cast<size_t>(R) * 256 + 1) * sizeof(uint32_t);
    switch ((K + 3) / 4) {  // K <= 28
    case 1: hipLaunchKernelGGL(locate_pairs_kernel<1>, grid, block, lds, st, a); break;
    case 2: hipLaunchKernelGGL(locate_pairs_kernel<2>, grid, block, lds, st, a); break;
    case 3: hipLaunchKernelGGL(locate_pairs_kernel<3>, grid, block, lds, st, a); break;
    case 4: hipLaunchKernelGGL(locate_pairs_kernel<4>, grid, block, lds, st, a); break;
    case 5: hipLaunchKernelGGL(locate_pairs_kernel<5>, grid, block, lds, st, a); break;
    case 6: hipLaunchKernelGGL(locate_pairs_kernel<6>, grid, block, lds, st, a); break;
    default: hipLaunchKernelGGL(locate_pairs_kernel<7>, grid, block, lds, st, a); break;
    }
    HIP_TRY(hipGetLastError());
    g_pairs_launches.fetch_add(1, std::memory_order_relaxed);
    hipLaunchKernelGGL(pairs_finalize_kernel, dim3(static_cast<unsigned>((nstripes + 255) / 256)), dim3(256), 0, st, d_pairs,
                       nstripes);
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
// stream: correct_kernel and, with d_counts, the counts.  Nothing here waits for the stream or copies
// to the host -- the case of every stripe is decided on the device.  The grid as locate_pairs.
int correct_located(const std::vector<int>& A, int K, int R, const CorrectTable& t, uint8_t* base, int64_t stripe_stride,
                    const int64_t* in_off, const int64_t* chk_off, int64_t blocksize, int nstripes, const uint32_t* d_status,
                    const uint32_t* d_suspects, const uint32_t* d_pairs, uint32_t* d_counts, hipStream_t st)
{
    if (R >= 1 && R <= kPairsMaxRows && t.dev) {  // no checked fragment: every stripe reads clean
        CorrectArgs a{};
        a.base = base;
        a.status = d_status;
        a.suspects = d_suspects;
        a.pairs = t.pairs ? d_pairs : nullptr;
        a.table = t.dev;
        a.stripe_stride = stripe_stride;
        a.len = blocksize;
        for (int j = 0; j < K; j++) a.off[j] = in_off[j];
        for (int r = 0; r < R; r++) a.off[K + r] = chk_off[r];
        fill_cmask(A, K, R, a.cmask);
        a.nstripes = nstripes;
        a.K = K;
        a.P = K + R;
        int chunks = 0, slots = 0;
        stripe_grid((blocksize + 3) >> 2, nstripes, chunks, slots);
        const dim3 grid(static_cast<unsigned>(chunks), static_cast<unsigned>(slots)), block(256);
        switch ((K + 3) / 4) {  // K <= 31
        case 1: hipLaunchKernelGGL(correct_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(correct_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(correct_kernel<3>, grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL(correct_kernel<4>, grid, block, 0, st, a); break;
        case 5: hipLaunchKernelGGL(correct_kernel<5>, grid, block, 0, st, a); break;
        case 6: hipLaunchKernelGGL(correct_kernel<6>, grid, block, 0, st, a); break;
        case 7: hipLaunchKernelGGL(correct_kernel<7>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(correct_kernel<8>, grid, block, 0, st, a); break;
        }
        HIP_TRY(hipGetLastError());
        g_correct_launches.fetch_add(1, std::memory_order_relaxed);
    }
    if (d_counts) {
        hipLaunchKernelGGL(correct_counts_kernel, dim3(1), dim3(256), 0, st, d_status, d_suspects, d_pairs, nstripes, d_counts);
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

template <bool LOCATE, class Args>
void xor_check_launch(int groups, dim3 grid, dim3 block, hipStream_t st, const Args& a)
{
    // full stripes: 2 ((3,3,3): 6 fragments) to 7 ((20,6,4): 26); degraded: 1 (up to 4 participants) to 7
    switch (groups) {
    case 1:
        if constexpr (std::is_same_v<Args, XorCheckSlotArgs>) {
            hipLaunchKernelGGL((xor_check_kernel<1, LOCATE, Args>), grid, block, 0, st, a);
            break;
        }
        [[fallthrough]];
    case 2: hipLaunchKernelGGL((xor_check_kernel<2, LOCATE, Args>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((xor_check_kernel<3, LOCATE, Args>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL((xor_check_kernel<4, LOCATE, Args>), grid, block, 0, st, a); break;
    case 5: hipLaunchKernelGGL((xor_check_kernel<5, LOCATE, Args>), grid, block, 0, st, a); break;
    case 6: hipLaunchKernelGGL((xor_check_kernel<6, LOCATE, Args>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((xor_check_kernel<7, LOCATE, Args>), grid, block, 0, st, a); break;
    }
}

// Fused stage of ecamd_xor_check or, with d_suspects, of ecamd_xor_locate over the whole tiles of
// every fragment (fragment f at f*frag_stride; masks: the m parity bitmaps, sig: ecamd_xor_check_plan).
// Geometry as launch_xor: one-wave workgroups on 1 KiB tiles or 256-lane workgroups on 4 KiB tiles
// (knob xor_check_threads 64 / 256), one workgroup per tile, long batches as launches of
// xor_tiles_per_slot tiles (of 4 KiB) per slot with xor_wgs (0: 3) slots per CU.  By default one-wave
// tiles at every size, where launch_xor takes them from 256 KiB: on clean data they tie with 4 KiB tiles
// at (10,6,4) x 1 MiB (0.614 against 0.615 ms) and win every repetition at (3,3,3) x 4 KiB (0.473
// against 0.486 ms; tools/check_bench.py --xor, profiles/xor_check.json).  Returns
// the bytes of each fragment covered, or 0 with nothing launched when it declines: knob
// xor_check_fused 0, a fragment shorter than a tile, a stripe the 32-bit buffer offsets cannot span.
// xor_check_tiles is the part both argument forms share: `a` comes with its tables filled, `last` is the
// highest fragment index it loads.
template <class Args>
int64_t xor_check_tiles(int dev, Args& a, int last, const uint8_t* base, int64_t stripe_stride, int64_t frag_stride,
                        int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* d_suspects, void* stream)
{
    constexpr bool kSlots = std::is_same_v<Args, XorCheckSlotArgs>;
    if (!g_tune.xor_check_fused || nstripes <= 0) return 0;
    const int knob_threads = g_tune.xor_check_threads;
    const int threads = knob_threads ? knob_threads : 64;
    const int64_t tile = static_cast<int64_t>(threads) * 16;
    const int64_t cover = blocksize / tile * tile;
    if (cover == 0 || stripe_stride < 0) return 0;
    if (last * frag_stride + blocksize >= (int64_t(1) << 31)) return 0;
    const uint64_t tps = static_cast<uint64_t>(cover / tile);
    const int wgs_knob = g_tune.xor_wgs;
    const int wgs = wgs_knob > 0 ? wgs_knob : 3;
    const uint64_t slots = static_cast<uint64_t>(dev_cu_count(dev)) * static_cast<uint64_t>(wgs);
    const uint64_t limit = static_cast<uint64_t>(std::max<int>(g_tune.xor_tiles_per_slot, 0)) * static_cast<uint64_t>(256 / threads);
    const int per = launch_stripes(nstripes, tps, slots, limit);
    if (tps * static_cast<uint64_t>(per) > 0x7fffffffull) return 0;
    a.stripe_stride = stripe_stride;
    a.records = static_cast<uint32_t>(last * frag_stride + cover);
    a.tiles_per_stripe = static_cast<uint32_t>(tps);
    for (int i = 0; i < a.nfrags; i++) {
        int f = i;
        if constexpr (kSlots) f = a.slot_frag[i];
        a.off32[i] = static_cast<int32_t>(f * frag_stride);
    }
    const int groups = (a.nfrags + 3) / 4;
    const auto st = static_cast<hipStream_t>(stream);
    for (int s0 = 0; s0 < nstripes; s0 += per) {
        const int ns = std::min(per, nstripes - s0);
        a.base = base + s0 * stripe_stride;
        a.status = d_status + s0;
        a.suspects = d_suspects ? d_suspects + s0 : nullptr;
        const dim3 grid(static_cast<unsigned>(tps * static_cast<uint64_t>(ns))), block(static_cast<unsigned>(threads));
        if (d_suspects)
            xor_check_launch<true>(groups, grid, block, st, a);
        else
            xor_check_launch<false>(groups, grid, block, st, a);
        HIP_TRY(hipGetLastError());
        (d_suspects ? g_xor_locate_fused : g_xor_check_fused).fetch_add(1, std::memory_order_relaxed);
    }
    return cover;
}

int64_t xor_check_fused(int dev, int k, int m, const uint32_t* masks, const uint32_t* sig, const uint8_t* base,
                        int64_t stripe_stride, int64_t frag_stride, int64_t blocksize, int nstripes, uint32_t* d_status,
                        uint32_t* d_suspects, void* stream)
{
    const int n = k + m;
    if (n <= 4 || n > kXorCheckMaxFrags || m > kXorCheckMaxRows) return 0;
    XorCheckArgs a{};
    a.nfrags = n;
    a.nrows = m;
    a.k = k;
    for (int f = 0; f < n; f++) a.sig[f] = sig[f];
    for (int p = 0; p < m; p++) a.masks[p] = masks[p] | (1u << (k + p));
    return xor_check_tiles(dev, a, n - 1, base, stripe_stride, frag_stride, blocksize, nstripes, d_status, d_suspects, stream);
}

// The slots of a degraded flat XOR plan (ecamd_xor_check_plan_degraded), what the degraded form of xor_check_kernel
// works on: the participants -- the available fragments that occur in a surviving row, ascending --
// and the surviving rows packed densely in the order of their owners.
struct XorSlots {
    std::vector<int> frag;        // fragment index of slot i
    std::vector<uint32_t> masks;  // packed row r over slot numbers
    std::vector<uint32_t> sig;    // slot i over packed rows
    std::vector<int> row_bit;     // status bit of packed row r: k + its owner
};

// The same stage for a degraded stripe: only the participants are loaded, in (participants + 3) / 4
// groups.  Declines as xor_check_fused does, and for a plan without a surviving row.
int64_t xor_check_fused_slots(int dev, const XorSlots& sl, const uint8_t* base, int64_t stripe_stride, int64_t frag_stride,
                              int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* d_suspects, void* stream)
{
    const int n = static_cast<int>(sl.frag.size()), rows = static_cast<int>(sl.masks.size());
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
        a.row_bit[r] = static_cast<uint8_t>(sl.row_bit[static_cast<size_t>(r)]);
    }
    return xor_check_tiles(dev, a, sl.frag.back(), base, stripe_stride, frag_stride, blocksize, nstripes, d_status, d_suspects,
                           stream);
}

// What the entry points differ in.  Fragment f of stripe s lies at base + s*stripe_stride +
// f*frag_stride.
struct CheckPlan {
    std::vector<int> inputs, checked;     // fragment indices of the K inputs and the R checked fragments
    const std::vector<int>* A = nullptr;  // R x K over GF(2^16): checked row r = sum of A[r][j] * input j
    // what computes the checked rows into the scratch
    const ecamd_map* map = nullptr;  // rs_vand: ecamd_map_apply_strided; whole tiles take the fused stage
    std::vector<uint32_t> masks;     // flat XOR: ecamd_xor_apply_strided over the parity bitmaps; whole tiles take
    std::vector<uint32_t> sig;       //   xor_check_fused with the signatures of ecamd_xor_check_plan
    CheckMap cached;                 // what A and map point into: the cached check map (rs_vand)
    PairsTable pairs;                //   and its pair table (ecamd_rs_locate_pairs)
    CorrectTable correct;            // the correction table (ecamd_rs_correct: with the cached map; flat XOR: xor_correct_table)
    std::vector<int> bitmaps;        // or the parity bitmaps as 0 / 1 (flat XOR)
    // flat XOR with fragments missing (xor_degraded_call): masks and bitmaps are the reduced rows over
    // `inputs`, sig stays empty and whole tiles take xor_check_fused_slots over these
    bool degraded = false;
    XorSlots slots;
};

// Bytes [from, bs) of the checked fragments at off[] (bit bits[r] each) of every stripe against what
// the plan's apply computes from the inputs at in_off[].  `from` a multiple of 16.  With `loc` (its
// map tables, input bits and suspects filled in) the compare step is locate_compare_kernel, which
// writes the status bits too.
int check_generic(int dev, void* stream, const CheckPlan& p, const uint8_t* base, int64_t stripe_stride,
                  const int64_t* in_off, const int64_t* off, const uint8_t* bits, int64_t from, int64_t bs, int nstripes,
                  uint32_t* d_status, const LocateCmpArgs* loc)
{
    const int nrows = static_cast<int>(p.checked.size());
    if (from >= bs || nrows <= 0 || nstripes <= 0) return 0;
    if (nrows > 32) return dev_fail(ECAMD_EINVAL, "check of %d fragments", nrows);
    const auto st = static_cast<hipStream_t>(stream);
    const int64_t cap = static_cast<int64_t>(kCheckScratchBytes);
    const int64_t seg = std::max<int64_t>(65536, cap / nrows / 65536 * 65536);  // fragment bytes per pass
    for (int64_t f0 = from; f0 < bs; f0 += seg) {
        const int64_t len = std::min(seg, bs - f0);
        const int64_t pitch = (len + 255) & ~int64_t(255);
        const int per = static_cast<int>(std::min<int64_t>(std::clamp<int64_t>(cap / (pitch * nrows), 1, 65535), nstripes));
        uint32_t* scratch = nullptr;
        int rc = stream_scratch(dev, stream, kCheckScratchSlot, static_cast<size_t>(per) * nrows * pitch / 4, &scratch);
        if (rc) return rc;
        auto* calc = reinterpret_cast<uint8_t*>(scratch);
        std::vector<int64_t> io(in_off, in_off + p.inputs.size()), oo;
        for (auto& v : io) v += f0;
        for (int r = 0; r < nrows; r++) oo.push_back(r * pitch);
        for (int s0 = 0; s0 < nstripes; s0 += per) {
            const int ns = std::min(per, nstripes - s0);
            const uint8_t* in = base + s0 * stripe_stride;
            rc = p.map ? ecamd_map_apply_strided(p.map, in, stripe_stride, io.data(), calc, nrows * pitch, oo.data(), len, ns, stream)
                       : ecamd_xor_apply_strided(p.masks.data(), nrows, static_cast<int>(io.size()), in, stripe_stride, io.data(),
                                                 calc, nrows * pitch, oo.data(), len, ns, stream);
            if (rc) return rc;
            // the fields both compare kernels take
            auto common = [&](auto& a, uint8_t* row_bit) {
                a.base = base + s0 * stripe_stride + f0;
                a.calc = calc;
                a.status = d_status + s0;
                a.stripe_stride = stripe_stride;
                a.pitch = pitch;
                a.len = len;
                a.nrows = nrows;
                for (int r = 0; r < nrows; r++) {
                    a.off[r] = off[r];
                    row_bit[r] = bits[r];
                }
            };
            if (loc) {
                LocateCmpArgs l = *loc;
                common(l, l.row_bit);
                l.suspects = loc->suspects + s0;
                const unsigned lx = static_cast<unsigned>(std::clamp<int64_t>((((len + 15) >> 4) + 1023) / 1024, 1, 1024));
                hipLaunchKernelGGL(locate_compare_kernel, dim3(lx, static_cast<unsigned>(ns)), dim3(256), 0, st, l);
            } else {
                CheckCmpArgs c{};
                common(c, c.bit);
                const unsigned gx = static_cast<unsigned>(std::clamp<int64_t>(((len >> 4) + 1023) / 1024, 1, 1024));
                hipLaunchKernelGGL(check_compare_kernel, dim3(gx, static_cast<unsigned>(nrows), static_cast<unsigned>(ns)),
                                   dim3(256), 0, st, c);
            }
            HIP_TRY(hipGetLastError());
        }
    }
    return 0;
}

// The layout checks of every entry point and, for a locate, its own two.
int check_layout(bool locate, const void* base, int64_t stripe_stride, int64_t frag_stride, int64_t blocksize,
                 int nstripes, const uint32_t* d_status, const uint32_t* d_suspects)
{
    if (!base || !d_status || nstripes < 0 || blocksize < 1 || frag_stride < blocksize)
        return dev_fail(ECAMD_EINVAL, "bad base / status / blocksize / strides");
    if ((reinterpret_cast<uintptr_t>(base) & 15u) || stripe_stride % 16 || frag_stride % 16)
        return dev_fail(ECAMD_EINVAL, "fragment addresses must be 16-byte aligned");
    if (locate && !d_suspects) return dev_fail(ECAMD_EINVAL, "null suspects");
    // an odd size ends in half a word, whose product is cut to 8 bits: proportionality cannot be tested
    if (locate && (blocksize & 1))
        return dev_fail(ECAMD_EINVAL, "locate needs an even blocksize (%lld)", static_cast<long long>(blocksize));
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

// The check (d_suspects null) or locate of one validated call: both arrays set, the fused stage over
// whole tiles, the generic stage over the rest, the finalize step of a locate and, with d_pairs, the
// pair stage on its results and, with fix_base (the same address as base, writable: ecamd_rs_correct,
// ecamd_xor_correct), the correction on both.  StreamUse: the scratch of the stream context outlives
// the call.
int run_check(int dev, const CheckPlan& p, const void* base, int64_t stripe_stride, int64_t frag_stride,
              int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* d_suspects, void* stream,
              uint32_t* d_pairs = nullptr, void* fix_base = nullptr, uint32_t* d_counts = nullptr)
{
    if (nstripes == 0) return 0;
    const StreamUse use(dev, stream);
    const auto st = static_cast<hipStream_t>(stream);
    const size_t words = static_cast<size_t>(nstripes) * sizeof(uint32_t);
    if (d_suspects) HIP_TRY(hipMemsetAsync(d_suspects, 0xff, words, st));
    HIP_TRY(hipMemsetAsync(d_status, 0, words, st));
    const int K = static_cast<int>(p.inputs.size()), R = static_cast<int>(p.checked.size());
    const auto* b = static_cast<const uint8_t*>(base);
    std::vector<int64_t> in_off, chk_off;
    std::vector<uint8_t> in_bits, bits;
    uint32_t participating = 0;
    for (int i : p.inputs) {
        in_off.push_back(i * frag_stride);
        in_bits.push_back(static_cast<uint8_t>(i));
        participating |= 1u << i;
    }
    for (int f : p.checked) {
        chk_off.push_back(f * frag_stride);
        bits.push_back(static_cast<uint8_t>(f));
        participating |= 1u << f;
    }
    // fewer than 2 checked fragments tell nothing apart: the check, then every participating
    // fragment of a dirty stripe
    const bool locating = d_suspects && R >= 2;
    auto fused = [&](int row0, int nrows) {
        return check_fused(dev, *p.A, K, row0, nrows, b, stripe_stride, in_off.data(), chk_off.data(), bits.data(), d_status,
                           locating ? d_suspects : nullptr, in_bits.data(), blocksize, nstripes, stream);
    };
    // whole tiles through the fused kernel; what it covered is done, the rest of each fragment goes
    // the generic way
    int64_t cover = 0;
    if (p.map && locating) {
        // one launch over all R rows: the second stage needs every row's syndrome in one wave, so
        // more than 8 rows are declined and take the generic stage alone
        cover = fused(0, R);
    } else if (p.map) {
        // one launch per group of 8 rows; only what EVERY group covered is done
        cover = blocksize;
        for (int row0 = 0; row0 < R && cover >= 0; row0 += 8) cover = std::min(cover, fused(row0, std::min(8, R - row0)));
    } else if (!p.sig.empty()) {
        // flat XOR: one launch reads all K + R fragments of a tile and takes the syndromes from the loads
        cover = xor_check_fused(dev, K, R, p.masks.data(), p.sig.data(), b, stripe_stride, frag_stride, blocksize, nstripes,
                                d_status, locating ? d_suspects : nullptr, stream);
    } else if (p.degraded) {
        // the same over the participants of the reduced rows alone
        cover = xor_check_fused_slots(dev, p.slots, b, stripe_stride, frag_stride, blocksize, nstripes, d_status,
                                      locating ? d_suspects : nullptr, stream);
    }
    if (cover < 0) return static_cast<int>(cover);
    LocateCmpArgs loc{};
    if (locating) {
        loc.suspects = d_suspects;
        locate_tables(*p.A, R, K, loc);
        for (int j = 0; j < K; j++) loc.in_bit[j] = in_bits[static_cast<size_t>(j)];
    }
    const int rc = check_generic(dev, stream, p, b, stripe_stride, in_off.data(), chk_off.data(), bits.data(), cover,
                                 blocksize, nstripes, d_status, locating ? &loc : nullptr);
    if (rc || !d_suspects) return rc;
    hipLaunchKernelGGL(locate_finalize_kernel, dim3(static_cast<unsigned>((nstripes + 255) / 256)), dim3(256), 0, st,
                       d_status, d_suspects, participating, nstripes, d_pairs);
    HIP_TRY(hipGetLastError());
    if (d_pairs && R >= 4) {  // fewer than four checks leave d_pairs zero
        const int prc = locate_pairs(*p.A, K, R, p.pairs, b, stripe_stride, in_off.data(), chk_off.data(), blocksize, nstripes,
                                     d_status, d_suspects, d_pairs, st);
        if (prc) return prc;
    }
    if (!fix_base) return 0;
    return correct_located(*p.A, K, R, p.correct, static_cast<uint8_t*>(fix_base), stripe_stride, in_off.data(), chk_off.data(),
                           blocksize, nstripes, d_status, d_suspects, d_pairs, d_counts, st);
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

// ecamd_rs_check (locate false), ecamd_rs_locate and ecamd_rs_locate_pairs (pairs true): a bad layout
// is reported before too many missing fragments, so it is checked before the plan is made.
int rs_call(bool locate, int k, int m, const int* missing, const void* base, int64_t stripe_stride, int64_t frag_stride,
            int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* d_suspects, uint32_t* checked, void* stream,
            bool pairs = false, uint32_t* d_pairs = nullptr, void* fix_base = nullptr, uint32_t* d_counts = nullptr)
{
    int dev = 0;
    int rc = dev_ensure(&dev);
    if (rc) return rc;
    if (k <= 0 || m < 0 || k + m > 32)
        return dev_fail(ECAMD_EINVAL, "%s needs k + m <= 32 (k=%d m=%d)", locate ? "locate" : "check", k, m);
    if ((rc = check_layout(locate, base, stripe_stride, frag_stride, blocksize, nstripes, d_status, d_suspects))) return rc;
    if (pairs && !d_pairs) return dev_fail(ECAMD_EINVAL, "null pairs");
    CheckPlan p;
    if ((rc = check_map(k, m, missing, p.cached))) return rc;
    if (pairs && (rc = check_map_pairs(p.cached, p.pairs))) return rc;
    if (fix_base && (rc = check_map_correct(p.cached, p.correct))) return rc;
    p.inputs = *p.cached.inputs;
    p.checked = *p.cached.checked;
    p.A = p.cached.coeff;
    p.map = p.cached.map;
    uint32_t mask = 0;
    for (int f : p.checked) mask |= 1u << f;
    if (checked) *checked = mask;  // for an empty batch too
    return run_check(dev, p, base, stripe_stride, frag_stride, blocksize, nstripes, d_status, locate ? d_suspects : nullptr,
                     stream, pairs ? d_pairs : nullptr, fix_base, d_counts);
}

// The correction table of a flat XOR code (CorrectTable above) from its check plan:
// fragment f is participant f, its pivot the lowest row of sig[f], every scale 1.  Device memory made
// at the first call that asks, per (device, k, m, hd, mask of lost fragments), and kept for the life of
// the process (a few accepted codes and the loss patterns a caller meets, 128 bytes each).  With
// fragments lost (`plan` degraded) fragment f is the participant correct_kernel loads in its place --
// its index among plan.inputs, or K + r for the owner of packed row r -- and its pivot the packed row
// of the lowest bit of sig[f]; a fragment no surviving row contains takes no part.
int xor_correct_table(int dev, int k, int m, int hd, uint32_t lost, const std::vector<uint32_t>& sig, const CheckPlan& plan,
                      CorrectTable& out)
{
    static std::mutex mu;
    static std::map<std::array<int, 5>, const uint32_t*> tables;
    const std::lock_guard<std::mutex> lk(mu);
    const uint32_t*& slot = tables[{dev, k, m, hd, static_cast<int>(lost)}];
    if (!slot) {
        uint32_t tab[32];
        for (int f = 0; f < 32; f++)
            tab[f] = f < k + m && sig[static_cast<size_t>(f)]
                         ? static_cast<uint32_t>(f) | static_cast<uint32_t>(__builtin_ctz(sig[static_cast<size_t>(f)])) << 8 | 1u << 16
                         : 0xffffffffu;
        if (plan.degraded) {
            const int K = static_cast<int>(plan.inputs.size()), R = static_cast<int>(plan.checked.size());
            for (int f = 0; f < k + m; f++) {
                if (tab[f] == 0xffffffffu) continue;
                int part = -1, row = -1;
                for (int j = 0; j < K; j++)
                    if (plan.inputs[static_cast<size_t>(j)] == f) part = j;
                for (int r = 0; r < R; r++) {
                    if (plan.checked[static_cast<size_t>(r)] == f) part = K + r;
                    if (row < 0 && plan.checked[static_cast<size_t>(r)] == k + __builtin_ctz(sig[static_cast<size_t>(f)])) row = r;
                }
                tab[f] = part < 0 || row < 0 ? 0xffffffffu : static_cast<uint32_t>(part) | static_cast<uint32_t>(row) << 8 | 1u << 16;
            }
        }
        const void* d = nullptr;  // once per code, before anything is enqueued
        if (const int rc = upload_table("correction table", tab, sizeof(tab), &d)) return rc;
        slot = static_cast<const uint32_t*>(d);
    }
    out.dev = slot;
    out.pairs = false;
    return 0;
}

// ecamd_xor_check (locate false) and ecamd_xor_locate: the parity bitmaps as a 0 / 1 map over GF(2^16).
int xor_call(bool locate, int k, int m, int hd, const void* base, int64_t stripe_stride, int64_t frag_stride,
             int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* d_suspects, void* stream,
             void* fix_base = nullptr, uint32_t* d_counts = nullptr)
{
    int dev = 0;
    int rc = dev_ensure(&dev);
    if (rc) return rc;
    unsigned pb[32], db[32];
    if (k <= 0 || m <= 0 || k + m > 32 || ecamd_xor_code_tables(k, m, hd, pb, db) != 0)
        return dev_fail(ECAMD_EINVAL, "not a flat_xor_hd code: k=%d m=%d hd=%d", k, m, hd);
    if ((rc = check_layout(locate, base, stripe_stride, frag_stride, blocksize, nstripes, d_status, d_suspects))) return rc;
    CheckPlan p;
    p.masks.assign(pb, pb + m);
    p.sig.resize(static_cast<size_t>(k + m));
    if (ecamd_xor_check_plan(k, m, hd, p.sig.data()) != 0) return dev_fail(ECAMD_EINVAL, "no check plan: k=%d m=%d hd=%d", k, m, hd);
    for (int j = 0; j < k; j++) p.inputs.push_back(j);
    for (int r = 0; r < m; r++) {
        p.checked.push_back(k + r);
        for (int j = 0; j < k; j++) p.bitmaps.push_back((pb[r] >> j) & 1u);
    }
    p.A = &p.bitmaps;
    if (fix_base && (rc = xor_correct_table(dev, k, m, hd, 0u, p.sig, p, p.correct))) return rc;
    return run_check(dev, p, base, stripe_stride, frag_stride, blocksize, nstripes, d_status, locate ? d_suspects : nullptr,
                     stream, nullptr, fix_base, d_counts);
}

// ecamd_xor_check_degraded (locate false), ecamd_xor_locate_degraded and ecamd_xor_correct_degraded: the
// rows of ecamd_xor_check_plan_degraded as a check plan.  The owner parity of each surviving row is
// checked, every other participant -- the parities of retired pivot rows among them -- is an input, and
// the map is the reduced rows over those inputs; a fragment that is lost, or that no surviving row
// contains, is in neither list, so no stage reads or writes its slot.
int xor_degraded_call(bool locate, int k, int m, int hd, const int* missing, const void* base, int64_t stripe_stride,
                      int64_t frag_stride, int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* d_suspects,
                      uint32_t* covered, void* stream, void* fix_base = nullptr, uint32_t* d_counts = nullptr)
{
    int dev = 0;
    int rc = dev_ensure(&dev);
    if (rc) return rc;
    unsigned rows[32], sig[32], cov = 0;
    if (k <= 0 || m <= 0 || k + m > 32 || ecamd_xor_check_plan_degraded(k, m, hd, missing, rows, sig, &cov) < 0)
        return dev_fail(ECAMD_EINVAL, "not a flat_xor_hd code (k=%d m=%d hd=%d) or a bad list of missing fragments", k, m, hd);
    if ((rc = check_layout(locate, base, stripe_stride, frag_stride, blocksize, nstripes, d_status, d_suspects))) return rc;
    uint32_t lost = 0;
    if (missing)
        for (int i = 0; missing[i] > -1; i++) lost |= 1u << missing[i];
    CheckPlan p;
    p.degraded = true;
    for (int r = 0; r < m; r++)
        if (rows[r]) p.checked.push_back(k + r);
    for (int f = 0; f < k + m; f++) {
        if (!sig[f]) continue;
        p.slots.frag.push_back(f);
        if (!(f >= k && rows[f - k])) p.inputs.push_back(f);
    }
    const int K = static_cast<int>(p.inputs.size()), N = static_cast<int>(p.slots.frag.size());
    for (int f : p.checked) {
        const unsigned row = rows[f - k];
        uint32_t over_inputs = 0, over_slots = 0;
        for (int j = 0; j < K; j++) {
            const unsigned bit = (row >> p.inputs[static_cast<size_t>(j)]) & 1u;
            over_inputs |= bit << j;
            p.bitmaps.push_back(static_cast<int>(bit));
        }
        for (int i = 0; i < N; i++) over_slots |= ((row >> p.slots.frag[static_cast<size_t>(i)]) & 1u) << i;
        p.masks.push_back(over_inputs);
        p.slots.masks.push_back(over_slots);
        p.slots.row_bit.push_back(f);
    }
    for (int i = 0; i < N; i++) {
        const unsigned over_owners = sig[p.slots.frag[static_cast<size_t>(i)]];
        uint32_t packed = 0;  // the same over the surviving rows in their packed order
        for (size_t r = 0; r < p.checked.size(); r++) packed |= ((over_owners >> (p.checked[r] - k)) & 1u) << r;
        p.slots.sig.push_back(packed);
    }
    p.A = &p.bitmaps;
    if (fix_base && !p.checked.empty() &&
        (rc = xor_correct_table(dev, k, m, hd, lost, std::vector<uint32_t>(sig, sig + k + m), p, p.correct)))
        return rc;
    if (covered) *covered = cov;  // for an empty batch too
    return run_check(dev, p, base, stripe_stride, frag_stride, blocksize, nstripes, d_status, locate ? d_suspects : nullptr,
                     stream, nullptr, fix_base, d_counts);
}

// The host half of ecamd_rs_scrub, ecamd_xor_scrub and ecamd_rs_scrub_pairs, after the locate: a wait
// for `stream`, the arrays read back, the counts, and -- when a stripe has exactly one suspect --
// decode(lists) with lists[2*s..] = {f, -1} for such a stripe and {-1, -1} (the empty list) for every
// other.  With d_pairs the lists are 3 long: {f, -1, -1}, {a, b, -1} for a stripe with a pair, and
// the empty list.
template <class Decode>
int scrub_located(const uint32_t* d_status, const uint32_t* d_suspects, int nstripes, int* n_clean, int* n_repaired,
                  int* n_unlocated, void* stream, Decode&& decode, const uint32_t* d_pairs = nullptr,
                  int* n_repaired_pairs = nullptr)
{
    int clean = 0, repaired = 0, unlocated = 0, repaired_pairs = 0;
    const size_t width = d_pairs ? 3 : 2;
    if (nstripes > 0) {
        HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
        std::vector<uint32_t> status(static_cast<size_t>(nstripes)), suspects(static_cast<size_t>(nstripes));
        HIP_TRY(hipMemcpy(status.data(), d_status, status.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(suspects.data(), d_suspects, suspects.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        std::vector<uint32_t> pairs;
        if (d_pairs) {
            pairs.resize(static_cast<size_t>(nstripes));
            HIP_TRY(hipMemcpy(pairs.data(), d_pairs, pairs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
        std::vector<int> lists(static_cast<size_t>(nstripes) * width, -1);
        for (int s = 0; s < nstripes; s++) {
            const uint32_t sus = suspects[static_cast<size_t>(s)];
            const uint32_t pr = d_pairs ? pairs[static_cast<size_t>(s)] : 0u;
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
            const int rc = decode(lists.data());
            if (rc) return rc;
        }
    }
    if (n_clean) *n_clean = clean;
    if (n_repaired) *n_repaired = repaired;
    if (n_unlocated) *n_unlocated = unlocated;
    if (n_repaired_pairs) *n_repaired_pairs = repaired_pairs;
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

int ecamd_rs_check(int k, int m, const int* missing, const void* base, int64_t stripe_stride, int64_t frag_stride,
                   int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* checked, void* stream)
{
    return rs_call(false, k, m, missing, base, stripe_stride, frag_stride, blocksize, nstripes, d_status, nullptr, checked,
                   stream);
}

int ecamd_xor_check(int k, int m, int hd, const void* base, int64_t stripe_stride, int64_t frag_stride,
                    int64_t blocksize, int nstripes, uint32_t* d_status, void* stream)
{
    return xor_call(false, k, m, hd, base, stripe_stride, frag_stride, blocksize, nstripes, d_status, nullptr, stream);
}

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

int ecamd_rs_locate(int k, int m, const int* missing, const void* base, int64_t stripe_stride, int64_t frag_stride,
                    int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* d_suspects, uint32_t* checked,
                    void* stream)
{
    return rs_call(true, k, m, missing, base, stripe_stride, frag_stride, blocksize, nstripes, d_status, d_suspects, checked,
                   stream);
}

int ecamd_xor_locate(int k, int m, int hd, const void* base, int64_t stripe_stride, int64_t frag_stride,
                     int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* d_suspects, void* stream)
{
    return xor_call(true, k, m, hd, base, stripe_stride, frag_stride, blocksize, nstripes, d_status, d_suspects, stream);
}

int ecamd_rs_scrub(int k, int m, void* base, int64_t stripe_stride, int64_t frag_stride, int64_t blocksize,
                   int nstripes, uint32_t* d_status, uint32_t* d_suspects, int* n_clean, int* n_repaired,
                   int* n_unlocated, void* stream)
{
    if (m < 2) return dev_fail(ECAMD_EINVAL, "scrub needs m >= 2 to tell fragments apart (m=%d)", m);
    int rc = ecamd_rs_locate(k, m, nullptr, base, stripe_stride, frag_stride, blocksize, nstripes, d_status, d_suspects,
                             nullptr, stream);
    if (rc) return rc;
    return scrub_located(d_status, d_suspects, nstripes, n_clean, n_repaired, n_unlocated, stream, [&](const int* lists) {
        return ecamd_rs_decode_multi(k, m, lists, 2, 1, base, stripe_stride, frag_stride, blocksize, nstripes, stream);
    });
}

int ecamd_rs_locate_pairs(int k, int m, const int* missing, const void* base, int64_t stripe_stride, int64_t frag_stride,
                          int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* d_suspects, uint32_t* d_pairs,
                          uint32_t* checked, void* stream)
{
    return rs_call(true, k, m, missing, base, stripe_stride, frag_stride, blocksize, nstripes, d_status, d_suspects, checked,
                   stream, true, d_pairs);
}

int ecamd_rs_scrub_pairs(int k, int m, void* base, int64_t stripe_stride, int64_t frag_stride, int64_t blocksize,
                         int nstripes, uint32_t* d_status, uint32_t* d_suspects, uint32_t* d_pairs, int* n_clean,
                         int* n_repaired, int* n_repaired_pairs, int* n_unlocated, void* stream)
{
    if (m < 4) return dev_fail(ECAMD_EINVAL, "a pair repair needs m >= 4 (m=%d)", m);
    int rc = ecamd_rs_locate_pairs(k, m, nullptr, base, stripe_stride, frag_stride, blocksize, nstripes, d_status, d_suspects,
                                   d_pairs, nullptr, stream);
    if (rc) return rc;
    return scrub_located(
        d_status, d_suspects, nstripes, n_clean, n_repaired, n_unlocated, stream,
        [&](const int* lists) {
            return ecamd_rs_decode_multi(k, m, lists, 3, 1, base, stripe_stride, frag_stride, blocksize, nstripes, stream);
        },
        d_pairs, n_repaired_pairs);
}

long long ecamd_locate_pairs_launches(void) { return g_pairs_launches.load(std::memory_order_relaxed); }

int ecamd_xor_scrub(int k, int m, int hd, void* base, int64_t stripe_stride, int64_t frag_stride, int64_t blocksize,
                    int nstripes, uint32_t* d_status, uint32_t* d_suspects, int* n_clean, int* n_repaired,
                    int* n_unlocated, void* stream)
{
    int rc = ecamd_xor_locate(k, m, hd, base, stripe_stride, frag_stride, blocksize, nstripes, d_status, d_suspects, stream);
    if (rc) return rc;
    return scrub_located(d_status, d_suspects, nstripes, n_clean, n_repaired, n_unlocated, stream, [&](const int* lists) {
        return ecamd_xor_decode_multi(k, m, hd, lists, 2, 1, base, stripe_stride, frag_stride, blocksize, nstripes, stream);
    });
}

// Locate, then correct in place on the same stream: no wait for the stream, no copy to the host, no
// launch that depends on what the locate found -- correct_kernel reads the per-stripe words itself.
int ecamd_rs_correct(int k, int m, const int* missing, void* base, int64_t stripe_stride, int64_t frag_stride,
                     int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* d_suspects, uint32_t* d_pairs,
                     uint32_t* d_counts, uint32_t* checked, void* stream)
{
    return rs_call(true, k, m, missing, base, stripe_stride, frag_stride, blocksize, nstripes, d_status, d_suspects, checked,
                   stream, d_pairs != nullptr, d_pairs, base, d_counts);
}

int ecamd_xor_correct(int k, int m, int hd, void* base, int64_t stripe_stride, int64_t frag_stride, int64_t blocksize,
                      int nstripes, uint32_t* d_status, uint32_t* d_suspects, uint32_t* d_counts, void* stream)
{
    return xor_call(true, k, m, hd, base, stripe_stride, frag_stride, blocksize, nstripes, d_status, d_suspects, stream, base,
                    d_counts);
}

int ecamd_xor_check_degraded(int k, int m, int hd, const int* missing, const void* base, int64_t stripe_stride,
                             int64_t frag_stride, int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* covered,
                             void* stream)
{
    return xor_degraded_call(false, k, m, hd, missing, base, stripe_stride, frag_stride, blocksize, nstripes, d_status, nullptr,
                             covered, stream);
}

int ecamd_xor_locate_degraded(int k, int m, int hd, const int* missing, const void* base, int64_t stripe_stride,
                              int64_t frag_stride, int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* d_suspects,
                              uint32_t* covered, void* stream)
{
    return xor_degraded_call(true, k, m, hd, missing, base, stripe_stride, frag_stride, blocksize, nstripes, d_status,
                             d_suspects, covered, stream);
}

int ecamd_xor_correct_degraded(int k, int m, int hd, const int* missing, void* base, int64_t stripe_stride,
                               int64_t frag_stride, int64_t blocksize, int nstripes, uint32_t* d_status, uint32_t* d_suspects,
                               uint32_t* d_counts, uint32_t* covered, void* stream)
{
    return xor_degraded_call(true, k, m, hd, missing, base, stripe_stride, frag_stride, blocksize, nstripes, d_status,
                             d_suspects, covered, stream, base, d_counts);
}

long long ecamd_correct_launches(void) { return g_correct_launches.load(std::memory_order_relaxed); }

long long ecamd_xor_check_fused_launches(void) { return g_xor_check_fused.load(std::memory_order_relaxed); }
long long ecamd_xor_locate_fused_launches(void) { return g_xor_locate_fused.load(std::memory_order_relaxed); }

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

}  // extern "C"
