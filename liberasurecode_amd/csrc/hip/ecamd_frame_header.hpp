// ecamd_frame_header.hpp -- the 80-byte fragment header (fragment_header_t, include/erasurecode.h) as the
// framed calls stamp it: add_fragment_metadata (src/erasurecode_postprocessing.c:37-69) on a zeroed
// header (alloc_fragment_buffer, src/erasurecode_helpers.c:124-138).  Written once: plain C++ that
// crc_finalize_kernel (ecamd_frame.hip) and frame_stamp_masks_kernel (ecamd_frame_masks.hip) run on the
// device, ecamd_frame_header (host/host_api.cpp) runs on the host, and tests/c/frame_header.cpp checks
// there.  Also here: which fragment item j of a stripe of ecamd_frame_reconstruct_masks stamps.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define ECAMD_FRAME_HD __host__ __device__ __forceinline__
#else
#define ECAMD_FRAME_HD inline
#endif

namespace ecamd {

constexpr int kHeaderBytes = 80;            // sizeof(fragment_header_t)
constexpr int kMetaBytes = 59;              // sizeof(fragment_metadata_t)
constexpr uint32_t kFragMagic = 0xb0c5ecc;  // LIBERASURECODE_FRAG_HEADER_MAGIC
constexpr uint8_t kChksumCrc32 = 2;         // CHKSUM_CRC32
constexpr uint32_t kLibecVersion = (1u << 16) | (8u << 8);  // LIBERASURECODE_VERSION 1.8.0
constexpr uint32_t kBackendVersion = 1u << 16;              // ec_backend_version 1.0.0

// Byte offsets in the header: fragment_metadata_t (packed), then magic, libec_version, metadata_chksum.
constexpr int kHdrIdx = 0;              // uint32 idx
constexpr int kHdrSize = 4;             // uint32 size (payload bytes)
constexpr int kHdrBackendMetaSize = 8;  // uint32 frag_backend_metadata_size
constexpr int kHdrOrigDataSize = 12;    // uint64 orig_data_size
constexpr int kHdrChksumType = 20;      // uint8 chksum_type
constexpr int kHdrChksum = 21;          // uint32 chksum[0] (the payload CRC32); chksum[1..7] stay zero
constexpr int kHdrBackendId = 54;       // uint8 backend_id
constexpr int kHdrBackendVersion = 55;  // uint32 backend_version
constexpr int kHdrMagic = 59;           // uint32 magic
constexpr int kHdrLibecVersion = 63;    // uint32 libec_version
constexpr int kHdrMetaChksum = 67;      // uint32 metadata_chksum, over bytes [0, kMetaBytes)

// What every fragment of a framed call shares; fragment f of a stripe gets idx0 + f.
struct HeaderArgs {
    int write;
    int idx0;
    uint32_t size;
    uint32_t backend_meta_size;
    uint64_t orig_data_size;
    uint32_t backend_version;
    uint32_t libec_version;
    uint8_t chksum_type;
    uint8_t backend_id;
};

ECAMD_FRAME_HD HeaderArgs frame_header_args(int backend, int checksum, int64_t blocksize, uint64_t obj_size, int idx0)
{
    HeaderArgs h{};
    h.write = 1;
    h.idx0 = idx0;
    h.size = static_cast<uint32_t>(blocksize);
    h.backend_meta_size = 0;  // get_backend_metadata_size is 0 for both backends
    h.orig_data_size = obj_size;
    h.backend_version = kBackendVersion;
    h.libec_version = kLibecVersion;
    h.chksum_type = static_cast<uint8_t>(checksum);
    h.backend_id = static_cast<uint8_t>(backend);
    return h;
}

// A header is held as its 20 little-endian 32-bit words, w[i] = bytes 4i .. 4i+3: with the constant
// offsets below every access is to a word known at compile time, so a device thread keeps its header
// in registers and stores it as five 16-byte words of four.
constexpr int kHeaderWords = kHeaderBytes / 4;

// The low N bytes of v, little endian, into bytes off .. off+N-1 of a header whose bytes there are zero.
template <int N>
ECAMD_FRAME_HD void frame_put(uint32_t* w, int off, uint64_t v)
{
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int i = 0; i < N; ++i) w[(off + i) >> 2] |= static_cast<uint32_t>((v >> (8 * i)) & 0xffu) << (8 * ((off + i) & 3));
}

ECAMD_FRAME_HD uint32_t frame_byte(const uint32_t* w, int off) { return (w[off >> 2] >> (8 * (off & 3))) & 0xffu; }

// The little-endian 32-bit value at bytes off .. off+3.
ECAMD_FRAME_HD uint32_t frame_get32(const uint32_t* w, int off)
{
    uint32_t v = 0;
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) v |= frame_byte(w, off + i) << (8 * i);
    return v;
}

// One step of the checksum machine with byte table T (host/crc.hpp CrcMachine::step).
ECAMD_FRAME_HD uint32_t frame_crc_step(const uint32_t* T, uint32_t s, uint32_t b, int legacy)
{
    uint32_t sh = s >> 8;
    if (legacy && (s & 0x80000000u)) sh |= 0xff000000u;
    return T[(s ^ b) & 0xffu] ^ sh;
}

// The metadata checksum: the machine over the header's first kMetaBytes bytes.
ECAMD_FRAME_HD uint32_t frame_meta_crc(const uint32_t* T, const uint32_t* w, int legacy)
{
    uint32_t s = ~0u;
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int i = 0; i < kMetaBytes; ++i) s = frame_crc_step(T, s, frame_byte(w, i), legacy);
    return ~s;
}

// w[0..20) = the header of fragment idx: zeroed 80 bytes, the fields, the metadata checksum.  crc is
// stored when the checksum type is CRC32; any other type is stored, not computed.
ECAMD_FRAME_HD void frame_header_fill(uint32_t* w, const HeaderArgs& h, uint32_t idx, uint32_t crc, const uint32_t* T, int legacy)
{
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int i = 0; i < kHeaderWords; ++i) w[i] = 0u;
    frame_put<4>(w, kHdrIdx, idx);
    frame_put<4>(w, kHdrSize, h.size);
    frame_put<4>(w, kHdrBackendMetaSize, h.backend_meta_size);
    frame_put<8>(w, kHdrOrigDataSize, h.orig_data_size);
    frame_put<1>(w, kHdrChksumType, h.chksum_type);
    if (h.chksum_type == kChksumCrc32) frame_put<4>(w, kHdrChksum, crc);
    frame_put<1>(w, kHdrBackendId, h.backend_id);
    frame_put<4>(w, kHdrBackendVersion, h.backend_version);
    frame_put<4>(w, kHdrMagic, kFragMagic);
    frame_put<4>(w, kHdrLibecVersion, h.libec_version);
    frame_put<4>(w, kHdrMetaChksum, frame_meta_crc(T, w, legacy));
}

// ---- ecamd_frame_reconstruct_masks: item j of a stripe ----

// The j-th set bit of L, counted from bit 0; -1 when L has j or fewer bits.
ECAMD_FRAME_HD int frame_nth_set_bit(uint32_t L, int j)
{
    if (j < 0) return -1;
    for (int i = 0; i < j && L; ++i) L &= L - 1u;
    return L ? __builtin_ctz(L) : -1;
}

// The fragment that item j of a stripe stamps, from the stripe's mask L and the result word R the
// payload decode wrote for it (0 left alone, bit 31 unrecoverable, else the fragments rebuilt): the j-th
// lost fragment of a rebuilt stripe, -1 for nothing.  Whether a mask is recoverable is the decode's
// decision alone, read from R; f < nfrag only keeps a stamp inside its stripe whatever R holds.
ECAMD_FRAME_HD int frame_masks_target(uint32_t R, uint32_t L, int j, int nfrag)
{
    if (R == 0u || (R >> 31) != 0u) return -1;
    const int f = frame_nth_set_bit(L, j);
    return f < nfrag ? f : -1;
}

}  // namespace ecamd
