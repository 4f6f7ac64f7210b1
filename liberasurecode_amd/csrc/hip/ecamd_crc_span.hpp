// ecamd_crc_span.hpp -- the bodies the payload CRC32 kernels share (the algebra: host/crc.hpp; the image:
// build_crc_image): r0 of one span of a payload by one wave, the fold of a payload's span partials
// and tail bytes into its CRC32, and the store of a finished header.  crc_partial_kernel and
// crc_finalize_kernel (ecamd_frame.hip) run them over every fragment of a batch, crc_partial_masks_kernel
// and frame_stamp_masks_kernel (ecamd_frame_masks.hip) over the fragments device masks name.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ecamd_crc_dev.hpp"
#include "ecamd_frame.hpp"
#include "ecamd_isa.hpp"

namespace ecamd {
namespace crcdev {

// lane l takes lane l + N of its row of 16 (DPP row_shl; past the row's end: 0)
template <int N>
__device__ __forceinline__ uint32_t row_shl(uint32_t x)
{
    return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x100 + N, 0xf, 0xf, false));
}

// The image's prefix the span body looks up in LDS.  POS: position tables -- piece u of a group of 4
// has its own tables with the shift to the group's last piece (A^(1024*(3-u))) folded in, so the lane
// state takes one A^4096 step per 4 pieces instead of four A^1024 steps (a quarter of the serial
// lookup chain).
template <int MB, int G, bool POS>
struct SpanTables {
    static constexpr int PW = piece_words(MB), PIECE = POS ? 4 * PW : PW;
    static constexpr int FIELDS = (32 / G) << G, WORDS = PIECE + 7 * FIELDS;
};

// r0 of span q of the payload at p (a.body bytes in a.nspans spans of a.J KiB, aligned to the body's
// END), by one wave; tab: the staged tables.  The same value in every lane.
template <int MB, int G, bool POS>
__device__ __forceinline__ uint32_t span_r0(const CrcArgs& a, const uint32_t* tab, const uint8_t* p, int q, int lane)
{
    using TB = SpanTables<MB, G, POS>;
    constexpr int PW = TB::PW, PIECE = TB::PIECE, FIELDS = TB::FIELDS;
    const uint32_t* gap = tab + PIECE;
    const int64_t span = static_cast<int64_t>(a.J) * 1024;
    const int64_t start = a.body - static_cast<int64_t>(a.nspans - q) * span + lane * 16;
    uint32_t st = 0;
    // Two groups of 4 pieces in flight: group g+1 is loading while group g is looked up.  The
    // loads are unconditional buffer loads: a piece before the payload (the first span's
    // leading zeros) or past the span gets an out-of-range offset, which reads zeros with no
    // memory traffic, so the compiler can count the loads in flight (vmcnt(N), not vmcnt(0)).
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p), 0, static_cast<int>(a.body), 0x00020000);
    auto load4 = [&](int j, u32x4 (&v)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t off = start + static_cast<int64_t>(j + u) * 1024;
            const bool live = j + u < a.J && off >= 0;
            v[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, live ? static_cast<int>(off)
                                                                  : static_cast<int>(0x80000000u),
                                                         0, 2);
        }
    };
    u32x4 cur[4], nxt[4];
    load4(0, cur);
    for (int j = 0; j < a.J; j += 4) {
        load4(j + 4, nxt);
        if constexpr (POS) {
            st = xor3(lmap<G>(gap, st), piece_r0<MB>(tab, cur[0]), piece_r0<MB>(tab + PW, cur[1])) ^
                 piece_r0<MB>(tab + 2 * PW, cur[2]) ^ piece_r0<MB>(tab + 3 * PW, cur[3]);
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) st = lmap<G>(gap, st) ^ piece_r0<MB>(tab, cur[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
    }
    // Lane l's state sits (63 - l) pieces before the span end: fold pairs, quads, ... -- inside
    // each row of 16 lanes by DPP row_shl (lane l takes lane l + 2^t; only the lanes that are
    // multiples of 2^(t+1) matter), then the 4 row values by v_readlane, folded on uniform values
    // (no ds_bpermute: the LDS serves the lookups; broadcast lookups do not conflict)
    st = lmap<G>(tab + PIECE + FIELDS * 1, st) ^ row_shl<1>(st);
    st = lmap<G>(tab + PIECE + FIELDS * 2, st) ^ row_shl<2>(st);
    st = lmap<G>(tab + PIECE + FIELDS * 3, st) ^ row_shl<4>(st);
    st = lmap<G>(tab + PIECE + FIELDS * 4, st) ^ row_shl<8>(st);
    const uint32_t r0 = __builtin_amdgcn_readlane(st, 0), r1 = __builtin_amdgcn_readlane(st, 16);
    const uint32_t r2 = __builtin_amdgcn_readlane(st, 32), r3 = __builtin_amdgcn_readlane(st, 48);
    const uint32_t s0 = lmap<G>(tab + PIECE + FIELDS * 5, r0) ^ r1, s1 = lmap<G>(tab + PIECE + FIELDS * 5, r2) ^ r3;
    return lmap<G>(tab + PIECE + FIELDS * 6, s0) ^ s1;
}

// r0 of the payload at p from its a.nspans span partials pp (Horner with A^(J KiB), the image's span
// tables) and its last a.len - a.body bytes through the byte table; a.nspans > 0.
__device__ __forceinline__ uint32_t payload_r0(const CrcArgs& a, const uint32_t* img, const uint32_t* pp, const uint8_t* p)
{
    const uint32_t* span = img + a.span_off;
    const uint32_t* T = img + a.t_off;
    uint32_t acc = 0;
    for (int q = 0; q < a.nspans; ++q) {
        acc = span[acc & 0xff] ^ span[256 + ((acc >> 8) & 0xff)] ^ span[512 + ((acc >> 16) & 0xff)] ^
              span[768 + (acc >> 24)] ^ pp[q];
    }
    for (int64_t i = a.body; i < a.len; ++i) acc = frame_crc_step(T, acc, p[i], a.legacy);
    return acc;
}

// The header w (kHeaderWords words) to the fragment at out (16-byte aligned): five 16-byte stores.
__device__ __forceinline__ void store_header(uint8_t* out, const uint32_t* w)
{
#pragma unroll
    for (int c = 0; c < kHeaderWords / 4; ++c)
        *reinterpret_cast<uint4*>(out + 16 * c) = make_uint4(w[4 * c], w[4 * c + 1], w[4 * c + 2], w[4 * c + 3]);
}

}  // namespace crcdev
}  // namespace ecamd
