// ecamd_xor_masks_plan.hpp -- what ecamd_xor_decode_masks shares between the host and the device
// (DESIGN.md "Decode from device masks"): the entry of a flat_xor_hd code's decode table and the rank
// that finds a stripe's entry from its mask of lost fragments.  Plain C++: xor_decode_masks_kernel
// runs it on the device, ecamd_xor_decode_masks_plan (host/host_api.cpp) fills the table with it, and
// tests/c/xor_masks_plan.cpp checks both on the host against ecamd_xor_plan.
//
// The reference refuses every list of hd or more fragments (get_failure_pattern, GE_HD), and hd is 3
// or 4, so a code's recoverable patterns are the masks of at most hd - 1 <= 3 bits over its k + m <= 26
// fragments: at most 2952 of them, at (20,6,4).  The table holds one entry per pattern, the empty one
// included, at the pattern's rank.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define ECAMD_XOR_MASKS_HD __host__ __device__ __forceinline__
#else
#define ECAMD_XOR_MASKS_HD inline
#endif

namespace ecamd {

constexpr int kXorMasksMaxOut = 3;         // hd - 1 at most
constexpr int kXorMasksMaxEntries = 2952;  // (20,6,4): C(26,0) + C(26,1) + C(26,2) + C(26,3)
constexpr int32_t kXorMasksUnrecoverable = -1;

// One pattern of lost fragments, as xor_hd_decode with decode_parity 1 leaves the zero-filled lost
// slots: output out[r], r < n_out, is the XOR of the fragments in src[r].  The outputs are the lost
// fragments ascending, so the data come first and a decode without parity takes the leading outputs
// below k unchanged (the plan of decode_parity 0 is exactly those rows).  src[r] names surviving
// fragments only and is never empty.  Unused outputs and sources are 0.
struct XorMasksEntry {
    uint8_t n_out;
    uint8_t out[kXorMasksMaxOut];
    uint32_t src[kXorMasksMaxOut];
};
static_assert(sizeof(XorMasksEntry) == 16, "XorMasksEntry layout");

// Patterns of fewer than hd of n fragments: the entries of the table of a code with k + m = n.
ECAMD_XOR_MASKS_HD int32_t xor_masks_count(int n, int hd)
{
    int32_t c = 0, binom = 1;  // C(n, t)
    for (int t = 0; t < hd; t++) {
        c += binom;
        binom = binom * (n - t) / (t + 1);
    }
    return c;
}

// The rank of mask L among the patterns of a code with n = k + m <= 32 fragments and distance hd <= 4:
// kXorMasksUnrecoverable for a bit >= n or hd or more bits; otherwise, with t = popcount(L) and the bits
// f0 < f1 < f2, offset[t] + C(f0,1) + C(f1,2) + C(f2,3), offset[t] = sum of C(n,i) over i < t -- the
// combinatorial number system, a bijection of the masks of t bits onto [0, C(n,t)).  The empty mask has
// rank 0 and is the only one that has.
ECAMD_XOR_MASKS_HD int32_t xor_masks_rank(int n, int hd, uint32_t L)
{
    const int t = __builtin_popcount(L);
    if ((n < 32 && (L >> n) != 0u) || t >= hd || t > kXorMasksMaxOut) return kXorMasksUnrecoverable;
    int32_t rank = xor_masks_count(n, t);  // offset[t]
    uint32_t rest = L;
    for (int i = 1; i <= t; i++) {
        const int32_t f = __builtin_ctz(rest);
        rest &= rest - 1u;
        rank += i == 1 ? f : i == 2 ? f * (f - 1) / 2 : f * (f - 1) * (f - 2) / 6;
    }
    return rank;
}

}  // namespace ecamd
