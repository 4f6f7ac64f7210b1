// frame_header.cpp -- csrc/hip/ecamd_frame_header.hpp (the header text crc_finalize_kernel and the stamp
// kernel of ecamd_frame_reconstruct_masks run on the device) compiled stand-alone with g++ and compared
// with a header packed here field by field from the wire format (include/erasurecode.h:
// fragment_metadata_t, fragment_header_t), through ecamd_frame_header and through frame_header_fill;
// and the helper that picks item j's fragment from a stripe's mask, for every j over a sweep of masks.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "crc.hpp"
#include "ecamd_frame_header.hpp"
#include "ecamd_host.h"

using namespace ecamd;

namespace {

int g_fail = 0;
long g_headers = 0, g_masks = 0;

void fail(const char* what, long a, long b)
{
    if (g_fail++ < 20) std::printf("%s (%ld, %ld)\n", what, a, b);
}

#pragma pack(push, 1)
struct WireMeta {
    uint32_t idx, size, backend_meta_size;
    uint64_t orig_data_size;
    uint8_t chksum_type;
    uint32_t chksum[8];
    uint8_t chksum_mismatch, backend_id;
    uint32_t backend_version;
};
struct WireHeader {
    WireMeta meta;
    uint32_t magic, libec_version, metadata_chksum;
    uint8_t pad[9];
};
#pragma pack(pop)
static_assert(sizeof(WireMeta) == 59 && sizeof(WireHeader) == 80, "wire format");

// bit by bit, no table: zlib's crc32, or the legacy variant whose shift drags bit 31 into the top byte
uint32_t slow_crc(const uint8_t* p, size_t n, bool legacy)
{
    uint32_t s = ~0u;
    for (size_t i = 0; i < n; i++) {
        uint32_t t = (s ^ p[i]) & 0xffu;
        for (int b = 0; b < 8; b++) t = (t & 1u) ? 0xEDB88320u ^ (t >> 1) : t >> 1;
        uint32_t sh = s >> 8;
        if (legacy && (s & 0x80000000u)) sh |= 0xff000000u;
        s = t ^ sh;
    }
    return ~s;
}

void check_header(int idx, uint32_t bs, uint64_t obj_size, int backend, int checksum, uint32_t crc, bool legacy)
{
    WireHeader want;
    std::memset(&want, 0, sizeof want);
    want.meta.idx = static_cast<uint32_t>(idx);
    want.meta.size = bs;
    want.meta.orig_data_size = obj_size;
    want.meta.chksum_type = static_cast<uint8_t>(checksum);
    if (checksum == 2) want.meta.chksum[0] = crc;
    want.meta.backend_id = static_cast<uint8_t>(backend);
    want.meta.backend_version = 1u << 16;
    want.magic = 0xb0c5ecc;
    want.libec_version = (1u << 16) | (8u << 8);
    want.metadata_chksum = slow_crc(reinterpret_cast<const uint8_t*>(&want.meta), sizeof want.meta, legacy);

    uint8_t got[80];
    std::memset(got, 0xEE, sizeof got);
    if (ecamd_frame_header(idx, bs, obj_size, backend, checksum, crc, legacy ? 1 : 0, got) != 0) fail("ecamd_frame_header failed", idx, checksum);
    if (std::memcmp(got, &want, 80) != 0) fail("ecamd_frame_header differs", idx, checksum);

    // the shared text itself, idx through idx0 + f as the kernels pass it
    const CrcMachine mach(legacy);
    uint32_t w[kHeaderWords];
    const HeaderArgs h = frame_header_args(backend, checksum, bs, obj_size, 1);
    frame_header_fill(w, h, static_cast<uint32_t>(h.idx0 + idx - 1), crc, mach.t, legacy ? 1 : 0);
    for (int i = 0; i < kHeaderBytes; i++)
        if (frame_byte(w, i) != reinterpret_cast<const uint8_t*>(&want)[i]) fail("frame_header_fill differs at byte", i, idx);
    if (frame_get32(w, kHdrMagic) != kFragMagic || frame_get32(w, kHdrMetaChksum) != want.metadata_chksum ||
        frame_get32(w, kHdrIdx) != static_cast<uint32_t>(idx) || frame_get32(w, kHdrSize) != bs ||
        frame_meta_crc(mach.t, w, legacy ? 1 : 0) != want.metadata_chksum)
        fail("frame_get32 / frame_meta_crc", idx, checksum);
    g_headers++;
}

// frame_nth_set_bit and frame_masks_target against a bit-by-bit walk.
void check_mask(uint32_t L, int nfrag)
{
    int bits[32], n = 0;
    for (int f = 0; f < 32; f++)
        if ((L >> f) & 1u) bits[n++] = f;
    for (int j = -1; j <= 33; j++) {
        const int want = j >= 0 && j < n ? bits[j] : -1;
        if (frame_nth_set_bit(L, j) != want) fail("frame_nth_set_bit", static_cast<long>(L), j);
        const uint32_t rebuilt = static_cast<uint32_t>(n);
        const int inside = want >= 0 && want < nfrag ? want : -1;
        // a rebuilt stripe: the j-th lost fragment, never one at or past nfrag whatever the words hold
        if (n && frame_masks_target(rebuilt, L, j, nfrag) != inside) fail("frame_masks_target (rebuilt)", static_cast<long>(L), j);
        // left alone, or unrecoverable: nothing
        if (frame_masks_target(0u, L, j, nfrag) != -1) fail("frame_masks_target (result 0)", static_cast<long>(L), j);
        if (frame_masks_target(0x80000000u | rebuilt, L, j, nfrag) != -1) fail("frame_masks_target (unrecoverable)", static_cast<long>(L), j);
    }
    g_masks++;
}

}  // namespace

int main()
{
    const uint32_t crcs[] = {0u, 0xdeadbeefu, 0xffffffffu, 0x80000001u};
    for (int backend : {6, 3})
        for (int legacy = 0; legacy < 2; legacy++)
            for (int checksum : {1, 2, 3})
                for (int idx : {1, 13, 27, 31})
                    for (uint64_t obj_size : {uint64_t(1), uint64_t(10) << 20, (uint64_t(1) << 32) + 5})
                        for (uint32_t bs : {2u, 1000u, 1u << 20, 0x7ffffffeu})
                            for (uint32_t crc : crcs) check_header(idx, bs, obj_size, backend, checksum, crc, legacy != 0);
    uint8_t out[80];
    if (ecamd_frame_header(0, 2, 2, 6, 2, 0, 0, nullptr) != -1 || ecamd_frame_header(-1, 2, 2, 6, 2, 0, 0, out) != -1)
        fail("ecamd_frame_header accepts bad arguments", 0, 0);

    // every mask of (10,4) and (3,3): k + m = 14 and 6 bits, bits at and past k + m included
    for (uint32_t L = 0; L < (1u << 16); L++) check_mask(L, 14);
    for (uint32_t L = 0; L < (1u << 8); L++) check_mask(L, 6);
    // wide masks: single bits, runs from either end, a seeded walk
    for (int f = 0; f < 32; f++) {
        check_mask(1u << f, 28);
        check_mask(0xffffffffu << f, 28);
        check_mask(0xffffffffu >> f, 32);
    }
    uint32_t x = 0x9e3779b9u;
    for (int i = 0; i < 20000; i++) {
        x = x * 1664525u + 1013904223u;
        check_mask(x, 26);
        check_mask(x & (x >> 7) & (x << 5), 28);  // sparse: a few bits, as real masks are
    }
    if (g_fail) {
        std::printf("frame_header: %d failures\n", g_fail);
        return 1;
    }
    std::printf("frame_header: ok (%ld headers, %ld masks)\n", g_headers, g_masks);
    return 0;
}
