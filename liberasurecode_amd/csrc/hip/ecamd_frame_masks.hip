// ecamd_frame_masks.hip -- the stamp stage of ecamd_frame_reconstruct_masks (DESIGN.md "Whole fragments
// from device masks"): the payload CRC32 and the 80-byte header of every fragment the payload decode
// (ecamd_rs_decode_masks / ecamd_xor_decode_masks) has just rebuilt, named by the same device mask words.
//
// Two launches on the caller's stream behind the decode, whatever the masks hold:
//   crc_partial_masks_kernel<MB, G, POS>  with CRC32 checksums only.  One wave per item (stripe s, j <
//                          jmax, span q).  The wave reads result[s] and lost[s] as scalars, takes f = the
//                          j-th set bit of lost[s] (frame_masks_target, ecamd_frame_header.hpp) and leaves
//                          on a scalar branch when the stripe was not rebuilt or has fewer than j + 1 lost
//                          fragments: such an item costs those two word loads and no payload traffic.
//                          Otherwise span q of fragment f's payload through crc_partial_kernel's body
//                          (crcdev::span_r0, ecamd_crc_span.hpp), on the same image and knobs.
//   frame_stamp_masks_kernel  one thread per (s, j): the same two words and f; the fold of the item's span
//                          partials and tail bytes (crcdev::payload_r0, as crc_finalize_kernel), the
//                          header's text (frame_header_fill, as crc_finalize_kernel), five 16-byte stores.
// jmax is min(m, 8) (rs_vand) or hd - 1 (flat_xor_hd): the most fragments a rebuilt stripe can have
// lost, so neither the grids nor the partials scale with k + m.  Whether a stripe was rebuilt is read
// from the decode's result word; the rule itself lives in the decode kernels alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ecamd.h"
#include "ecamd_crc_span.hpp"
#include "ecamd_frame.hpp"
#include "ecamd_internal.hpp"

namespace ecamd {

namespace {

// A value that is the same in every lane of the wave, in a scalar register.
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ uint8_t* stamp_frag(const CrcArgs& a, int64_t s, int f)
{
    return const_cast<uint8_t*>(a.base) + s * a.stripe_stride + static_cast<int64_t>(f) * a.frag_stride;
}

}  // namespace

template <int MB, int G, bool POS>
__global__ __launch_bounds__(512) void crc_partial_masks_kernel(const CrcArgs a, const StampArgs sa,
                                                                const uint32_t* __restrict__ img,
                                                                uint32_t* __restrict__ partial)
{
    constexpr int WORDS = crcdev::SpanTables<MB, G, POS>::WORDS;
    __shared__ uint32_t tab[WORDS];
    for (int i = threadIdx.x; i < WORDS; i += blockDim.x) tab[i] = img[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t nw = blockDim.x >> 6;
    const uint32_t per = static_cast<uint32_t>(sa.jmax) * static_cast<uint32_t>(a.nspans);  // items per stripe
    const int64_t total = static_cast<int64_t>(sa.nstripes) * per;
    // the wave's index is the same in all its lanes: everything derived from it below is scalar
    for (int64_t ws = static_cast<int64_t>(blockIdx.x) * nw + uniform(threadIdx.x >> 6); ws < total;
         ws += static_cast<int64_t>(gridDim.x) * nw) {
        const int64_t s = ws / per;
        const uint32_t r = static_cast<uint32_t>(ws - s * per);
        const int j = static_cast<int>(r / static_cast<uint32_t>(a.nspans));
        const int q = static_cast<int>(r - static_cast<uint32_t>(j) * static_cast<uint32_t>(a.nspans));
        const int f = frame_masks_target(uniform(sa.result[s]), uniform(sa.lost[s]), j, a.nfrag);
        if (f < 0) continue;  // scalar: nothing of this item's stripe was rebuilt, or fewer than j + 1 fragments
        const uint32_t st = crcdev::span_r0<MB, G, POS>(a, tab, stamp_frag(a, s, f) + a.payload_off, q, lane);
        if (lane == 0) partial[ws] = st;
    }
}

__global__ __launch_bounds__(128) void frame_stamp_masks_kernel(const CrcArgs a, const StampArgs sa,
                                                                const uint32_t* __restrict__ img,
                                                                const uint32_t* __restrict__ partial, const HeaderArgs h)
{
    const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;  // s * jmax + j
    if (t >= static_cast<int64_t>(sa.nstripes) * sa.jmax) return;
    const int64_t s = t / sa.jmax;
    const int j = static_cast<int>(t - s * sa.jmax);
    const int f = frame_masks_target(sa.result[s], sa.lost[s], j, a.nfrag);
    if (f < 0) return;
    uint8_t* frag = stamp_frag(a, s, f);
    uint32_t crc = 0;
    if (a.nspans > 0) crc = ~(a.c0 ^ crcdev::payload_r0(a, img, partial + t * a.nspans, frag + a.payload_off));
    uint32_t hd[kHeaderWords];
    frame_header_fill(hd, h, static_cast<uint32_t>(h.idx0 + f), crc, img + a.t_off, a.legacy);
    crcdev::store_header(frag, hd);
}

int frame_stamp_masks(const CrcArgs& a, const CrcForm& form, const uint32_t* d_img, const StampArgs& sa, uint32_t* partial,
                      const HeaderArgs& h, unsigned grid, void* stream)
{
    const auto st = static_cast<hipStream_t>(stream);
    const int64_t items = static_cast<int64_t>(sa.nstripes) * sa.jmax;
    if (items <= 0) return 0;
    if (a.nspans > 0) {
        if (!partial) return dev_fail(ECAMD_EINVAL, "stamp stage: CRC32 spans without their scratch");
        with_crc_form(form, [&](auto mb, auto g, auto p) {
            hipLaunchKernelGGL((crc_partial_masks_kernel<decltype(mb)::value, decltype(g)::value, decltype(p)::value>),
                               dim3(grid), dim3(512), 0, st, a, sa, d_img, partial);
        });
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(frame_stamp_masks_kernel, dim3(static_cast<unsigned>((items + 127) / 128)), dim3(128), 0, st, a, sa,
                       d_img, partial, h);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace ecamd
