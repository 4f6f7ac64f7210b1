// ecamd_launch.hpp -- what the launch files (ecamd_device.hip, ecamd_small.hip, ecamd_rs.hip,
// ecamd_copy.hip) share that needs a kernel argument type: the map, launch geometry, the launchers of
// ecamd_device.hip and ecamd_small.hip, and the cached rs_vand map entry of ecamd_rs.hip.  Everything
// free of kernel types is in ecamd_internal.hpp.  A launch file includes this and gets the HIP runtime,
// ecamd.h, ecamd_internal.hpp and ecamd_kernels.hpp with it.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "../host/bitslice.hpp"
#include "ecamd.h"
#include "ecamd_internal.hpp"
#include "ecamd_kernels.hpp"

struct ecamd_map {
    struct Pass {
        int row0, width, col0, ncols;
        size_t offset;  // into d_tables: byte-split image
        size_t bytes;
        size_t nib_offset;  // nibble image (build_nibble_tables)
        size_t nib_bytes;
    };
    int device = 0;
    int R = 0, K = 0;
    std::vector<Pass> passes;
    uint8_t* d_tables = nullptr;
    std::vector<int> coeff;  // R x K (host copy: the bitsliced kernels are generated from it)
    // this map's identity for whatever caches its tables (the resident small server's slots): from a
    // process-wide counter at creation, never reused -- d_tables' address is, once the map is destroyed
    uint64_t serial = 0;
};

namespace ecamd {

// ---- ecamd_jit.hip: the bitsliced kernels' code objects ----
hipFunction_t bitslice_function(int dev, const std::vector<int>& coeff, int R, int K, int depth, bool wait,
                                std::shared_ptr<void>& hold, bool copy = false, int crc = 0, bool wave = false,
                                const std::vector<int>* in_shift = nullptr, int prefetch = 0, int* status = nullptr,
                                const BsOcc* occ = nullptr, bool check = false, bool locate = false, int opts = 0);
int bitslice_prebuild(const std::vector<int>& coeff, int R, int K, int depth, bool copy, int crc, bool wave,
                      const std::vector<int>* in_shift, int prefetch, const BsOcc& occ, const std::string& arch,
                      const std::string& dir, bool check = false, bool locate = false, int opts = 0);
int bitslice_launch(hipFunction_t fn, const BsArgs& args, int grid, hipStream_t st,
                    const std::shared_ptr<void>& hold, int threads = 256, unsigned lds = 0);

// ---- ecamd_device.hip: applying a map ----
struct Geometry {
    int threads;
    int grid;
    size_t lds;
    uint32_t tiles_per_stripe;
    uint32_t ntiles;
};
// Workgroup size, grid and tile counts of a pass of `lds` bytes of tables per workgroup over nstripes
// fragments of bs bytes, each thread taking `chunks` 16-byte chunks per tile; ECAMD_EINVAL past 2^32 tiles.
int geometry(int dev, size_t lds, int64_t bs, int nstripes, Geometry& g, int chunks = 1, int max_threads = 1024,
             int max_wgs = 8, int grid_mult = 1);
// Fill the 32-bit offsets and buffer sizes the stream kernels address a stripe by (a.in_off / out_off,
// a.copy_off); false when an offset is negative or past 2^31.
bool stream_offsets(ApplyArgs& a, int64_t bs);
bool stream_copy_offsets(ApplyArgs& a, int64_t bs);
// One strided LDS-table stream pass over a batch, split into launches of tiles_per_slot tiles per slot.
int launch_stream_pass(ApplyArgs a, int dev, size_t lds_bytes, int width, int ch, bool nib, int64_t bs, int nstripes,
                       hipStream_t st);

// Whether a row group of nrows outputs over K inputs takes the bitsliced kernel under the current
// knobs, and in which form (launch_bitslice; ecamd_bitslice_prebuild and ecamd_rs_kernel_form ask
// the same question without launching).
struct BsForm {
    bool wave = false;  // one-wave 4 KiB tiles (else 4-wave 16 KiB tiles)
    int depth = 0;      // LDS ring depth (0: register loads)
    int prefetch = 0;   // BitsliceStyle::prefetch (copy-through forms)
    BsOcc occ;          // one-wave forms: occupancy (knobs bs_wave_wmin / bs_wave_wmax / bs_wave_barrier)
    int opts = 0;       // plain one-wave register form: kBsOpt* bits (knob bs_store_through, ecamd_bitslice_timeline)
};
bool bs_form(int nrows, int K, bool copy, bool unaligned, BsForm& f);
// Lanes per workgroup of a form (a tile is 64 bytes of each fragment per lane).
int bs_threads(const BsForm& f);
// One-wave 4 KiB tiles for a bitsliced row group of `nrows` outputs (knobs bs_wave, bs_wave_min_rows,
// bs_wave_copy); `narrow`: the group takes the bitsliced kernel below bitslice_min_rows for it.
bool bs_wave_tiles(int nrows, int K, bool copy, bool* narrow, bool unaligned = false);
// The dynamic LDS a launch of the module kernel fn adds so that at most n of its workgroups are resident
// per CU: 0 when n is 0 or the static share is already that large.
unsigned cap_lds(hipFunction_t fn, int n);

// chk (ecamd_rs_check): the map is a syndrome matrix [A | I] whose last nrows inputs are the stored
// fragments under test; the check form of the kernel writes no fragment (out_off unused) and ORs
// bit chk->bits[r] into chk->status[stripe] for every row r whose syndrome is not zero.
// With `suspects` (ecamd_rs_locate) the kernel is the locate form: a wave that sees a non-zero syndrome
// also ANDs the mask of the candidates that explain it into suspects[stripe]; frag_bits[i] is the
// fragment index of the map's input i (the K inputs, then the checked rows).
struct BsCheck {
    uint32_t* status;
    const uint8_t* bits;
    uint32_t* suspects = nullptr;
    const uint8_t* frag_bits = nullptr;
};
// The bitsliced form of output rows [row0, row0 + nrows) of `map` over the whole tiles of every
// fragment; returns the bytes of each fragment it covered (0: not taken), *rc an error.
int64_t launch_bitslice(const ecamd_map* map, int row0, int nrows, const ApplyArgs& base, const int64_t* in_off,
                        const int64_t* out_off, int64_t bs, int nstripes, hipStream_t st, int* rc,
                        const int64_t* copy_off = nullptr, const BsCheck* chk = nullptr);
// Every pass of `map` over a batch: strided fragments (PTRS false: base_args' bases, strides and
// optional stripe list) or pointer tables (PTRS true).  Instantiated for both in ecamd_device.hip.
template <bool PTRS>
int launch_gf16(const ecamd_map* map, ApplyArgs base_args, const int64_t* in_off, const int64_t* out_off,
                int64_t bs_all, int nstripes, hipStream_t st);
// The same for a flat-XOR map of R masks over K inputs.
// copy_off (framed flat-XOR encode): input j is also stored at base_args.copy_base + s*copy_stride +
// copy_off[j] by the first row group's launches -- whole stream-kernel tiles only: ECAMD_EINVAL, with
// nothing launched, unless bs is a multiple of the tile and every offset fits the stream kernel.
template <bool PTRS>
int launch_xor(const uint32_t* masks, int R, int K, ApplyArgs base_args, const int64_t* in_off,
               const int64_t* out_off, int64_t bs, int nstripes, hipStream_t st, const int64_t* copy_off = nullptr);

// ---- ecamd_small.hip: launches of a few KiB ----
struct SmallCrcReq;  // the fused checksum of a small launch (ecamd_small.hip)
// A pass small enough for gf16_small_kernel: at most small_chunks 16-byte chunks in all, plain
// strided fragments (no copy-through, padding limits or stripe list) at one 16-byte aligned pitch
// per side.
bool small_launch(const ApplyArgs& a, int64_t bs, int nstripes);
// ECAMD_EINVAL (nothing launched) when `crc` is given and the launch cannot fuse it.  `last`: this launch
// ends the operation (the completion flag may be attached to it); `only`: it is the whole operation (then
// it may be posted to the resident small server).
int launch_small(const ApplyArgs& a, const ecamd_map::Pass& p, int64_t bs, int nstripes, const uint8_t* tables,
                 uint64_t serial, hipStream_t st, const SmallCrcReq* crc = nullptr, bool last = false,
                 bool only = false);
int launch_xor_small(const ApplyArgs& a, int64_t bs, int nstripes, hipStream_t st, bool last = false,
                     const SmallCrcReq* crc = nullptr, bool only = false);

// ---- ecamd_rs.hip: the cached rs_vand maps ----
// A prepared map with the fragment indices of its inputs and outputs.  Check maps (kind 4) also own the
// device tables of the check stages (ecamd_check.hip builds them on demand): freed with the entry, not
// counted against the cache's byte limit.
struct RsEntry {
    std::unique_ptr<ecamd_map, void (*)(ecamd_map*)> map{nullptr, ecamd_map_destroy};
    std::vector<int> inputs, outputs;
    OnceTable pairs, correct;
};
// The cached entry of (device, kind, k, m, rebuild, dest, missing): kind 0 encode, 1 decode, 2
// reconstruct, 4 check (rs_vand_plan's kinds).
int rs_entry(int kind, int k, int m, const int* missing, int rebuild, int dest, std::shared_ptr<RsEntry>& out);
// The cached entry (kind 3) of a flat-XOR decode-join map: `coeff` (outputs x inputs, 0 / 1) made a map
// at the first call and kept like the rs_vand ones.
int xor_join_entry(int dev, int k, const std::vector<int>& inputs, const std::vector<int>& outputs,
                   const std::vector<int>& coeff, std::shared_ptr<RsEntry>& out);

}  // namespace ecamd
