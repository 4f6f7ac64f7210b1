// ecamd_copy.hip -- the copy-through launches behind the framed calls of ecamd_frame_api.hip: an encode
// that reads objects and writes the data payloads as they stream through (rs_encode_copy,
// xor_encode_copy), the same with the payload CRC32s folded in (rs_encode_copy_crc, *_encode_copy_crc_bs,
// crc_encode_prebuild), and a decode straight into objects (rs_decode_join, xor_decode_join).  Contracts
// in ecamd_internal.hpp.  No state of its own: maps come from ecamd_rs.hip, launchers from
// ecamd_device.hip.
#include <algorithm>

#include "../host/gf16.hpp"
#include "../host/tune.hpp"
#include "ecamd_frame.hpp"
#include "ecamd_launch.hpp"

using namespace ecamd;

namespace {

// Copy-through launch of a cached rs map: input j of stripe s at in_base + s*in_stride +
// in_off[j] (map column order), output r at out_base + s*out_stride + out_off[r]; the first row
// group also stores input j at copy_base + s*copy_stride + copy_off[j] when copy_off[j] >= 0.
int map_apply_copy(const RsEntry& e, const uint8_t* in_base, int64_t in_stride,
                   const std::vector<int64_t>& in_off, uint8_t* out_base, int64_t out_stride,
                   const std::vector<int64_t>& out_off, uint8_t* copy_base, int64_t copy_stride,
                   const std::vector<int64_t>& copy_off, int64_t bs, int nstripes, void* stream,
                   const std::vector<int64_t>* in_len = nullptr,
                   const std::vector<int64_t>* out_len = nullptr,
                   const std::vector<int64_t>* copy_len = nullptr)
{
    const ecamd_map* map = e.map.get();
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto len_of = [&](const std::vector<int64_t>* v, int i) { return v ? (*v)[static_cast<size_t>(i)] : bs; };
    // Row groups of 5..8 outputs first take the bitsliced kernel over the whole 16 KiB tiles that
    // every input / copy / output fully holds (the first group copying the inputs through); the
    // LDS-table passes of those rows then run on the rest of each fragment only.
    std::vector<int64_t> bs_done(static_cast<size_t>((map->R + 7) / 8), 0);
    // knob frame_tail_fork: the LDS-table passes over each fragment's rest run on a side stream
    // beside the bitsliced launch (disjoint bytes) when that rest is 1-4 KiB -- one LDS-table launch
    // -- or, at 2, any rest; `pst` is the stream the passes go to
    hipStream_t pst = st;
    struct Joiner {  // error paths: the caller's stream still ends up after the side stream's work
        int dev;
        void* stream;
        bool on = false;
        ~Joiner()
        {
            if (on) (void)side_join(dev, stream);
        }
    } joiner{map->device, stream};
    {
        ApplyArgs b{};
        b.in_base = in_base;
        b.in_stride = in_stride;
        b.out_base = out_base;
        b.out_stride = out_stride;
        b.copy_base = copy_base;
        b.copy_stride = copy_stride;
        b.min_len = bs;
        for (int j = 0; j < map->K; j++) {
            b.min_len = std::min(b.min_len, len_of(in_len, j));
            if (copy_off[static_cast<size_t>(j)] >= 0) b.min_len = std::min(b.min_len, len_of(copy_len, j));
        }
        for (int r = 0; r < map->R; r++) b.min_len = std::min(b.min_len, len_of(out_len, r));
        b.limited = b.min_len < bs ? 1 : 0;
        // The bitsliced kernel covers whole 16 KiB tiles only; the rest of each fragment must then
        // run on the stream kernel (the pointer-free LDS-table kernels cannot start at an offset).
        // A row group whose passes cannot all take it (more than 20 inputs per pass, offsets past
        // 2 GiB) skips the bitsliced kernel instead of failing after writing part of the output.
        bool unaligned = false;
        for (int64_t o : in_off) unaligned = unaligned || (o & 15);
        auto cover_of = [&](int g) {  // bytes the group's bitsliced launch would cover
            const int64_t tile =
                bs_wave_tiles(std::min(8, map->R - g * 8), map->K, true, nullptr, unaligned) ? kBsTileWave : kBsTile;
            return (b.limited ? std::min<int64_t>(bs, b.min_len) : bs) / tile * tile;
        };
        auto tail_on_stream = [&](int g) {
            for (const auto& p : map->passes) {
                if (p.row0 / 8 != g) continue;
                if (p.ncols > 4 * kStreamGroups) return false;
                ApplyArgs t{};
                t.ncols = p.ncols;
                t.nrows = std::min(p.width, map->R - p.row0);
                for (int j = 0; j < p.ncols; j++) {
                    t.in_off[j] = in_off[p.col0 + j];
                    t.copy_off[j] = copy_off[p.col0 + j];
                }
                for (int r = 0; r < t.nrows; r++) t.out_off[r] = out_off[p.row0 + r];
                if (!stream_offsets(t, bs) || (p.row0 == 0 && !stream_copy_offsets(t, bs))) return false;
            }
            return true;
        };
        if (g_tune.stream && g_tune.frame_tail_fork != 0) {
            const int64_t rest = bs - cover_of(0);
            if (rest > 0 && rest < bs && (g_tune.frame_tail_fork == 2 || (rest >= 1024 && rest < 4096)) &&
                tail_on_stream(0)) {
                void* side = nullptr;
                const int rc = side_fork(map->device, stream, &side);
                if (rc) return rc;
                pst = static_cast<hipStream_t>(side);
                joiner.on = true;
            }
        }
        for (int g = 0; g * 8 < map->R && g_tune.stream; g++) {
            if (cover_of(g) < bs && !tail_on_stream(g)) continue;
            int brc = 0;
            b.copy_records = g == 0 ? 1 : 0;  // (recomputed from copy_off inside)
            bs_done[static_cast<size_t>(g)] =
                launch_bitslice(map, g * 8, std::min(8, map->R - g * 8), b, in_off.data(), out_off.data(), bs,
                                nstripes, st, &brc, g == 0 ? copy_off.data() : nullptr);
            if (brc) return brc;
        }
    }
    for (const auto& p : map->passes) {
        const int64_t done = bs_done[static_cast<size_t>(p.row0 / 8)];
        if (done >= bs) continue;
        const int64_t pbs = bs - done;  // this pass runs bytes [done, bs) of every fragment
        ApplyArgs a{};
        a.tables = map->d_tables + p.offset;
        a.in_base = in_base;
        a.in_stride = in_stride;
        a.out_base = out_base;
        a.out_stride = out_stride;
        a.copy_base = copy_base;
        a.copy_stride = copy_stride;
        a.bs = pbs;
        a.ncols = p.ncols;
        a.nrows = std::min(p.width, map->R - p.row0);
        a.accumulate = p.col0 > 0;
        auto rest = [&](int64_t len) { return static_cast<int32_t>(std::max<int64_t>(0, std::min(pbs, len - done))); };
        for (int j = 0; j < p.ncols; j++) {
            a.in_off[j] = in_off[p.col0 + j] + done;
            a.copy_off[j] = copy_off[p.col0 + j] < 0 ? -1 : copy_off[p.col0 + j] + done;
            a.in_len32[j] = rest(len_of(in_len, p.col0 + j));
            a.copy_len32[j] = rest(len_of(copy_len, p.col0 + j));
        }
        for (int r = 0; r < a.nrows; r++)
            a.out_len32[r] = rest(len_of(out_len, p.row0 + r));
        a.min_len = pbs;
        for (int j = 0; j < p.ncols; j++) {
            a.min_len = std::min<int64_t>(a.min_len, a.in_len32[j]);
            if (a.copy_off[j] >= 0) a.min_len = std::min<int64_t>(a.min_len, a.copy_len32[j]);
        }
        for (int r = 0; r < a.nrows; r++) a.min_len = std::min<int64_t>(a.min_len, a.out_len32[r]);
        a.limited = a.min_len < pbs ? 1 : 0;
        for (int r = 0; r < a.nrows; r++) a.out_off[r] = out_off[p.row0 + r] + done;
        Geometry g;
        int rc;
        if (g_tune.stream && p.ncols <= 4 * kStreamGroups && stream_offsets(a, pbs) &&
            (p.row0 != 0 || stream_copy_offsets(a, pbs))) {
            rc = launch_stream_pass(a, map->device, p.bytes, p.width, 1, false, pbs, nstripes, pst);
            if (rc) return rc;
            continue;
        }
        if (done > 0) return dev_fail(ECAMD_EINVAL, "copy-through tail needs 32-bit stream offsets");
        rc = geometry(map->device, p.bytes, bs, nstripes, g);
        if (rc) return rc;
        a.ntiles = g.ntiles;
        a.tiles_per_stripe = g.tiles_per_stripe;
        dim3 grid(g.grid), block(g.threads);
        if (p.row0 == 0) {  // the first row group copies the inputs through
            switch (p.width) {
            case 2: hipLaunchKernelGGL((gf16_copy_apply_kernel<2>), grid, block, g.lds, pst, a); break;
            case 4: hipLaunchKernelGGL((gf16_copy_apply_kernel<4>), grid, block, g.lds, pst, a); break;
            default: hipLaunchKernelGGL((gf16_copy_apply_kernel<8>), grid, block, g.lds, pst, a); break;
            }
        } else {
            switch (p.width) {
            case 2: hipLaunchKernelGGL((gf16_apply_kernel<2, false, true, false>), grid, block, g.lds, pst, a); break;
            case 4: hipLaunchKernelGGL((gf16_apply_kernel<4, false, true, false>), grid, block, g.lds, pst, a); break;
            default: hipLaunchKernelGGL((gf16_apply_kernel<8, false, true, false>), grid, block, g.lds, pst, a); break;
            }
        }
        HIP_TRY(hipGetLastError());
    }
    if (joiner.on) {
        joiner.on = false;
        return side_join(map->device, stream);
    }
    return 0;
}

bool copy_aligned(const void* obj, const void* payload0, int64_t obj_stride, int64_t stripe_stride,
                  int64_t frag_stride, int64_t bs)
{
    return aligned16(obj) && aligned16(payload0) && obj_stride % 16 == 0 &&
           stripe_stride % 16 == 0 && frag_stride % 16 == 0 && bs % 16 == 0;
}

// Copy-through encode from objects whose k chunks of bs bytes start at unaligned object offsets
// (j*bs, bs even but not a multiple of 16) and may end early (objects shorter than k*bs): the
// payload side stays 16-byte aligned, the object side is read with unaligned 16-byte loads.
bool copy_aligned_payloads(const void* obj, const void* payload0, int64_t obj_stride,
                           int64_t stripe_stride, int64_t frag_stride, int64_t bs)
{
    return aligned16(obj) && aligned16(payload0) && obj_stride % 16 == 0 && stripe_stride % 16 == 0 &&
           frag_stride % 16 == 0 && bs % 2 == 0;
}

// The crc variant's prefetch and (one-wave form) occupancy for an m-output encode map with crc_pos
// flags -- shared by the launch and the build-time prebuild, so both name the same code object.
int crc_form_args(int m, int crc_pos, BsOcc& occ)
{
    occ = BsOcc{};
    if (!(crc_pos & 32)) return m <= 4 ? static_cast<int>(g_tune.frame_crc_prefetch) : 0;
    occ.wmin = g_tune.frame_crc_wave_wpe > 0 ? static_cast<int>(g_tune.frame_crc_wave_wpe) : m > 4 ? 2 : 3;
    occ.wmax = occ.wmin;
    // (5-8 outputs: no registers for a second input ahead)
    return m > 4 && g_tune.frame_crc_wave_pf == 3 ? 4 : static_cast<int>(g_tune.frame_crc_wave_pf);
}

// The crc variant of the bitsliced kernel for the encode map `coeff` (m x k, row-major; RS
// generator rows or a flat-XOR code's 0/1 parity masks) on `device`: see rs_encode_copy_crc_bs.
int encode_copy_crc_bs(int device, const std::vector<int>& coeff, int k, int m, const void* obj, int64_t obj_stride,
                       void* payload0, int64_t stripe_stride, int64_t frag_stride, int64_t bs, int nstripes,
                       const uint32_t* d_img, uint32_t* d_partial, int q, void* stream, int crc_pos, int64_t cover)
{
    const int mode = g_tune.bitslice;
    if (cover < 0) cover = bs;
    // crc_pos & 32: one-wave 4 KiB tiles in workgroups of (crc_pos >> 6) waves, per-tile partials
    // (tile-major, q unused); else more than 4 outputs fold every 16 KiB tile on its own
    // (bitslice.cpp fold_each), q = tiles
    const int cw = (crc_pos & 32) ? (crc_pos >> 6) & 15 : 0;
    const int64_t tile = cw ? kBsTileWave : kBsTile;
    if (!mode || m > kBsMaxR || k > kBsMaxK || cover % tile || cover <= 0 || cover > bs || nstripes <= 0 ||
        (!cw && (q <= 0 || (cover / kBsTile) % q || (m > 4 && q != cover / kBsTile))))
        return ECAMD_EINVAL;
    // whole payloads: the object chunks j*bs are 16-byte aligned; partial cover (objects that do not
    // fill k 16 KiB-multiple payloads): the object side is read with unaligned loads
    if (!(cover == bs ? copy_aligned(obj, payload0, obj_stride, stripe_stride, frag_stride, bs)
                      : copy_aligned_payloads(obj, payload0, obj_stride, stripe_stride, frag_stride, bs)))
        return ECAMD_EINVAL;
    ApplyArgs a{};
    a.in_base = static_cast<const uint8_t*>(obj);
    a.in_stride = obj_stride;
    a.out_base = static_cast<uint8_t*>(payload0);
    a.out_stride = stripe_stride;
    a.copy_base = static_cast<uint8_t*>(payload0);
    a.copy_stride = stripe_stride;
    a.ncols = k;
    a.nrows = m;
    for (int j = 0; j < k; j++) {
        a.in_off[j] = j * bs;
        a.copy_off[j] = j * frag_stride;
    }
    for (int r = 0; r < m; r++) a.out_off[r] = (k + r) * frag_stride;
    if (!stream_offsets(a, bs) || !stream_copy_offsets(a, bs) || k > 254) return ECAMD_EINVAL;
    std::shared_ptr<void> hold;
    // crc_pos: position sets (1, 2, 4) + 8 for the lane-shift fold (which 5-8 outputs always take)
    // + 16 for nibble piece tables
    // the crc variant keeps unaligned loads for object chunks at offsets that are not multiples of
    // 16: the realigned form measured no faster there (Swift segments 1.496 vs 1.486 ms, 4 MiB
    // objects 1.544 vs 1.542, profiles/r04_cover_ab2.log) and its larger register need spills at
    // some shift patterns (C3 objects 10 bytes long), which then fall back to the codec + CRC pass
    const uint32_t in_records = a.in_records;
    BsOcc occ{};
    const int prefetch = crc_form_args(m, crc_pos, occ);
    hipFunction_t fn = bitslice_function(device, coeff, m, k, 0, mode == 2, hold, true, crc_pos, false,
                                         nullptr, prefetch, nullptr, cw ? &occ : nullptr);
    if (!fn) return ECAMD_EINVAL;
    BsArgs b{};
    b.in_base = a.in_base;
    b.out_base = a.out_base;
    b.in_stride = a.in_stride;
    b.out_stride = a.out_stride;
    b.in_records = in_records;
    b.out_records = a.out_records;
    b.tiles_per_stripe = static_cast<uint32_t>(cover / tile);
    b.ntiles = b.tiles_per_stripe * static_cast<uint32_t>(nstripes);
    for (int j = 0; j < k; j++) {
        b.in_off[j] = a.in_off32[j];
        b.copy_idx[j] = static_cast<uint8_t>(j);
    }
    for (int r = 0; r < m; r++) b.out_off[r] = a.out_off32[r];
    b.copy_base = a.copy_base;
    b.copy_stride = a.copy_stride;
    b.copy_records = a.copy_records;
    b.copy_step = static_cast<uint32_t>(frag_stride);
    b.crc_img = d_img;
    b.crc_partial = d_partial;
    b.crc_q = q;
    b.crc_per = cw ? 0 : static_cast<int32_t>(cover / kBsTile / q);
    b.crc_nfrag = k + m;
    if (cw) {  // the first `big` workgroups: per tiles per wave, covering ~frame_crc_wave_big % of the
        // tiles; the rest one tile per wave
        const int64_t per = std::max<int64_t>(1, g_tune.frame_crc_wave_per);
        const int64_t big = per > 1 ? static_cast<int64_t>(b.ntiles) * g_tune.frame_crc_wave_big / 100 / (cw * per) : 0;
        b.crc_q = static_cast<int32_t>(big);
        b.crc_per = static_cast<int32_t>(per);
        const int64_t rest = static_cast<int64_t>(b.ntiles) - big * per * cw;
        const int64_t grid = big + (rest + cw - 1) / cw;
        return bitslice_launch(fn, b, static_cast<int>(grid), static_cast<hipStream_t>(stream), hold, 64 * cw,
                               cap_lds(fn, static_cast<int>(g_tune.frame_crc_per_cu)));
    }
    const int64_t units = static_cast<int64_t>(nstripes) * q;
    // one work unit per workgroup by default: the dispatcher hands the next unit to whichever CU
    // frees a slot, which balances units better than a grid-stride loop over resident workgroups
    const int wgs = static_cast<int>(g_tune.frame_crc_bs_wgs);
    const int grid = static_cast<int>(
        wgs > 0 ? std::min<int64_t>(units, static_cast<int64_t>(dev_cu_count(device)) * wgs) : units);
    return bitslice_launch(fn, b, grid, static_cast<hipStream_t>(stream), hold, 256,
                           cap_lds(fn, static_cast<int>(g_tune.frame_crc_per_cu)));
}

// The encode map in the order the fused framed encodes assume: inputs 0 .. k-1, outputs k .. k+m-1.
bool systematic(const RsEntry& e, int k, int m)
{
    for (int j = 0; j < k; j++)
        if (e.inputs[j] != j) return false;
    for (int r = 0; r < m; r++)
        if (e.outputs[r] != k + r) return false;
    return true;
}

// A flat-XOR code as a GF(2^16) matrix of 0 / 1 (m x k): the bitsliced network of a coefficient 1 is the
// identity on the bit planes, so the network is the parity masks' XORs.
std::vector<int> xor_coeff(const uint32_t* masks, int k, int m)
{
    std::vector<int> coeff(static_cast<size_t>(m) * k, 0);
    for (int r = 0; r < m; r++)
        for (int j = 0; j < k; j++) coeff[static_cast<size_t>(r) * k + j] = (masks[r] >> j) & 1u;
    return coeff;
}

// The decode-join of a prepared map (rs_decode_join, xor_decode_join): e's outputs are data fragments,
// computed into their object chunks; its data inputs are copied there as they stream through.
int decode_join_entry(const RsEntry& e, int k, const void* payload0, int64_t stripe_stride, int64_t frag_stride,
                      void* obj, int64_t obj_stride, int64_t bs, int nstripes, void* stream, int64_t obj_size)
{
    const RsEntry* ep = &e;
    if (!ep->map || nstripes <= 0 || bs <= 0)
        return dev_fail(ECAMD_EINVAL, "decode-join needs at least one missing data fragment");
    if (obj_size < 0) obj_size = k * bs;
    if (obj_size > k * bs || !copy_aligned_payloads(obj, payload0, obj_stride, stripe_stride, frag_stride, bs))
        return dev_fail(ECAMD_EINVAL, "decode-join needs 16-byte aligned objects and payloads");
    // object chunk j = [j*bs, j*bs + len_j): shorter (or empty) past the object's end
    auto chunk = [&](int j) {
        return std::max<int64_t>(0, std::min<int64_t>(bs, obj_size - static_cast<int64_t>(j) * bs));
    };
    std::vector<int64_t> in_off, out_off, copy_off, out_len, copy_len;
    for (int i : ep->inputs) {
        in_off.push_back(static_cast<int64_t>(i) * frag_stride);
        copy_off.push_back(i < k ? static_cast<int64_t>(i) * bs : -1);  // parity is not copied
        copy_len.push_back(i < k ? chunk(i) : bs);
    }
    for (int o : ep->outputs) {
        out_off.push_back(static_cast<int64_t>(o) * bs);
        out_len.push_back(chunk(o));
    }
    auto* ob = static_cast<uint8_t*>(obj);
    return map_apply_copy(*ep, static_cast<const uint8_t*>(payload0), stripe_stride, in_off, ob,
                          obj_stride, out_off, ob, obj_stride, copy_off, bs, nstripes, stream, nullptr,
                          &out_len, &copy_len);
}

}  // namespace

namespace ecamd {

int rs_encode_copy(int k, int m, const void* obj, int64_t obj_stride, void* payload0,
                   int64_t stripe_stride, int64_t frag_stride, int64_t bs, int nstripes,
                   void* stream, int64_t obj_size, int64_t from, int64_t to)
{
    std::shared_ptr<RsEntry> e;
    int rc = rs_entry(0, k, m, nullptr, 0, -1, e);
    if (rc) return rc;
    if (!e->map || nstripes <= 0 || bs <= 0) return 0;
    if (obj_size < 0) obj_size = k * bs;
    if (obj_size > k * bs || !copy_aligned_payloads(obj, payload0, obj_stride, stripe_stride, frag_stride, bs))
        return dev_fail(ECAMD_EINVAL, "copy-through encode needs 16-byte aligned objects and payloads");
    if (to < 0) to = bs;
    if (from < 0 || from % 16 || to > bs || from >= to || (to < bs && to % 16))
        return dev_fail(ECAMD_EINVAL, "copy-through encode: bad range [%lld, %lld)", (long long)from, (long long)to);
    // bytes [from, to) of every payload: object chunk j from j*bs + from, payloads from + from
    const int64_t len = to - from;
    std::vector<int64_t> in_off, out_off, copy_off, in_len;
    for (int i : e->inputs) {
        in_off.push_back(static_cast<int64_t>(i) * bs + from);
        copy_off.push_back(static_cast<int64_t>(i) * frag_stride + from);
        in_len.push_back(std::min(len, std::max<int64_t>(
                                           0, std::min<int64_t>(bs, obj_size - static_cast<int64_t>(i) * bs) - from)));
    }
    for (int o : e->outputs) out_off.push_back(static_cast<int64_t>(o) * frag_stride + from);
    auto* p0 = static_cast<uint8_t*>(payload0);
    return map_apply_copy(*e, static_cast<const uint8_t*>(obj), obj_stride, in_off, p0,
                          stripe_stride, out_off, p0, stripe_stride, copy_off, len, nstripes, stream,
                          &in_len);
}

// LDS bytes of gf16_frame_crc_kernel for an RS(k, m) encode: the pass's split tables, the CRC image
// (byte tables for the first mb piece dwords) and the waves' state exchange.
size_t fused_crc_lds(int k, int m, int mb, bool nib)
{
    const int w = m <= 2 ? 2 : (m <= 4 ? 4 : 8);
    const int ns = 4 * ((k + 3) / 4) + w;
    return static_cast<size_t>(k) * (nib ? 64 : 512) * 2 * w + (static_cast<size_t>(crc_fused_words(mb)) + 8 * ns) * 4;
}

// rs_encode_copy with the payload CRC32 folded in (gf16_frame_crc_kernel): r0 of range r of
// payload f of stripe s lands in d_partial[(s*(k+m) + f)*q + r].  Returns ECAMD_EINVAL without
// launching when the shape does not fit the fused kernel (the caller then runs the split path).
int rs_encode_copy_crc(int k, int m, const void* obj, int64_t obj_stride, void* payload0,
                       int64_t stripe_stride, int64_t frag_stride, int64_t bs, int nstripes,
                       const uint32_t* d_img, uint32_t* d_partial, int q, void* stream, int mb, bool nib)
{
    constexpr int kThreads = 512;
    constexpr int64_t kTile = kThreads * 16;
    std::shared_ptr<RsEntry> e;
    int rc = rs_entry(0, k, m, nullptr, 0, -1, e);
    if (rc) return rc;
    if (!e->map || nstripes <= 0 || bs <= 0 || bs % kTile || q <= 0 || (bs / kTile) % q)
        return ECAMD_EINVAL;
    const ecamd_map* map = e->map.get();
    if (map->passes.size() != 1 || !copy_aligned(obj, payload0, obj_stride, stripe_stride, frag_stride, bs))
        return ECAMD_EINVAL;
    if (!systematic(*e, k, m)) return ECAMD_EINVAL;
    const auto& p = map->passes[0];
    ApplyArgs a{};
    a.tables = map->d_tables + (nib ? p.nib_offset : p.offset);
    a.in_base = static_cast<const uint8_t*>(obj);
    a.in_stride = obj_stride;
    a.out_base = static_cast<uint8_t*>(payload0);
    a.out_stride = stripe_stride;
    a.copy_base = static_cast<uint8_t*>(payload0);
    a.copy_stride = stripe_stride;
    a.bs = bs;
    a.ncols = k;
    a.nrows = m;
    for (int j = 0; j < k; j++) {
        a.in_off[j] = j * bs;
        a.copy_off[j] = j * frag_stride;
    }
    for (int r = 0; r < m; r++) a.out_off[r] = (k + r) * frag_stride;
    if (k > 4 * kStreamGroups || !stream_offsets(a, bs) || !stream_copy_offsets(a, bs)) return ECAMD_EINVAL;
    const int kg = (k + 3) / 4;
    const int ns = 4 * kg + p.width;
    if (mb != 1 && mb != 4) return ECAMD_EINVAL;
    if (nib && (!map->d_tables || p.nib_bytes == 0)) return ECAMD_EINVAL;
    const size_t lds = fused_crc_lds(k, m, mb, nib);
    if (lds != (nib ? p.nib_bytes : p.bytes) + (static_cast<size_t>(crc_fused_words(mb)) + 8 * ns) * 4)
        return ECAMD_EINVAL;
    if (lds > static_cast<size_t>(kLdsBytes)) return ECAMD_EINVAL;
    a.tiles_per_stripe = static_cast<uint32_t>(bs / kTile);
    a.ntiles = a.tiles_per_stripe * static_cast<uint32_t>(nstripes);
    FusedCrcArgs c{d_img, d_partial, q, static_cast<int>(bs / kTile) / q, k + m};
    const int64_t units = static_cast<int64_t>(nstripes) * q;
    const int wgs_knob = g_tune.frame_crc_wgs;
    const int want = wgs_knob > 0 ? wgs_knob : 2;
    const int wgs = std::max<int>(1, std::min<int>(want, kLdsBytes / static_cast<int>(lds)));
    const dim3 grid(static_cast<unsigned>(std::min<int64_t>(units, static_cast<int64_t>(dev_cu_count(map->device)) * wgs)));
    const dim3 block(kThreads);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define ECAMD_FUSED(W, MB, NIB)                                                                                  \
    switch (kg) {                                                                                                \
    case 1: hipLaunchKernelGGL((gf16_frame_crc_kernel<W, 1, MB, NIB>), grid, block, lds, st, a, c); break;        \
    case 2: hipLaunchKernelGGL((gf16_frame_crc_kernel<W, 2, MB, NIB>), grid, block, lds, st, a, c); break;        \
    case 3: hipLaunchKernelGGL((gf16_frame_crc_kernel<W, 3, MB, NIB>), grid, block, lds, st, a, c); break;        \
    case 4: hipLaunchKernelGGL((gf16_frame_crc_kernel<W, 4, MB, NIB>), grid, block, lds, st, a, c); break;        \
    default: hipLaunchKernelGGL((gf16_frame_crc_kernel<W, 5, MB, NIB>), grid, block, lds, st, a, c); break;       \
    }
#define ECAMD_FUSED_W(W)                                    \
    if (nib) {                                              \
        if (mb == 4) { ECAMD_FUSED(W, 4, true) } else { ECAMD_FUSED(W, 1, true) }    \
    } else {                                                \
        if (mb == 4) { ECAMD_FUSED(W, 4, false) } else { ECAMD_FUSED(W, 1, false) }  \
    }
    if (p.width == 2) {
        ECAMD_FUSED_W(2)
    } else if (p.width == 4) {
        ECAMD_FUSED_W(4)
    } else {
        ECAMD_FUSED_W(8)
    }
#undef ECAMD_FUSED_W
#undef ECAMD_FUSED
    HIP_TRY(hipGetLastError());
    return 0;
}

int rs_encode_copy_crc_bs(int k, int m, const void* obj, int64_t obj_stride, void* payload0,
                          int64_t stripe_stride, int64_t frag_stride, int64_t bs, int nstripes,
                          const uint32_t* d_img, uint32_t* d_partial, int q, void* stream, int crc_pos,
                          int64_t cover)
{
    if (!g_tune.bitslice || m > kBsMaxR || k > kBsMaxK) return ECAMD_EINVAL;
    std::shared_ptr<RsEntry> e;
    int rc = rs_entry(0, k, m, nullptr, 0, -1, e);
    if (rc) return rc;
    if (!e->map || !systematic(*e, k, m)) return ECAMD_EINVAL;
    return encode_copy_crc_bs(e->map->device, e->map->coeff, k, m, obj, obj_stride, payload0, stripe_stride,
                              frag_stride, bs, nstripes, d_img, d_partial, q, stream, crc_pos, cover);
}

int xor_encode_copy_crc_bs(const uint32_t* masks, int k, int m, const void* obj, int64_t obj_stride, void* payload0,
                           int64_t stripe_stride, int64_t frag_stride, int64_t bs, int nstripes,
                           const uint32_t* d_img, uint32_t* d_partial, int q, void* stream, int crc_pos,
                           int64_t cover)
{
    int dev = 0;
    int rc = dev_ensure(&dev);
    if (rc) return rc;
    if (!masks || !g_tune.bitslice || m > kBsMaxR || k > kBsMaxK) return ECAMD_EINVAL;
    return encode_copy_crc_bs(dev, xor_coeff(masks, k, m), k, m, obj, obj_stride, payload0, stripe_stride, frag_stride, bs, nstripes,
                              d_img, d_partial, q, stream, crc_pos, cover);
}

int xor_encode_copy(const uint32_t* masks, int k, int m, const void* obj, int64_t obj_stride, void* payload0,
                    int64_t stripe_stride, int64_t frag_stride, int64_t bs, int64_t cover, int nstripes, void* stream)
{
    int rc = dev_ensure(nullptr);
    if (rc) return rc;
    if (nstripes <= 0 || cover <= 0) return 0;
    if (!masks || k <= 0 || k > 32 || m <= 0 || cover > bs || cover % 4096 || !aligned16(obj) || obj_stride % 16 ||
        !aligned16(payload0) || stripe_stride % 16 || frag_stride % 16)
        return ECAMD_EINVAL;
    std::vector<int64_t> in_off(static_cast<size_t>(k)), copy_off(static_cast<size_t>(k)), out_off(static_cast<size_t>(m));
    for (int j = 0; j < k; j++) {
        in_off[static_cast<size_t>(j)] = static_cast<int64_t>(j) * bs;
        copy_off[static_cast<size_t>(j)] = static_cast<int64_t>(j) * frag_stride;
    }
    for (int r = 0; r < m; r++) out_off[static_cast<size_t>(r)] = static_cast<int64_t>(k + r) * frag_stride;
    ApplyArgs a{};
    a.in_base = static_cast<const uint8_t*>(obj);
    a.in_stride = obj_stride;
    a.out_base = static_cast<uint8_t*>(payload0);
    a.out_stride = stripe_stride;
    a.copy_base = static_cast<uint8_t*>(payload0);
    a.copy_stride = stripe_stride;
    return launch_xor<false>(masks, m, k, a, in_off.data(), out_off.data(), cover, nstripes,
                             static_cast<hipStream_t>(stream), copy_off.data());
}

int rs_decode_join(int k, int m, const int* missing, const void* payload0, int64_t stripe_stride,
                   int64_t frag_stride, void* obj, int64_t obj_stride, int64_t bs, int nstripes,
                   void* stream, int64_t obj_size)
{
    std::shared_ptr<RsEntry> e;
    int rc = rs_entry(1, k, m, missing, 0, -1, e);
    if (rc) return rc;
    return decode_join_entry(*e, k, payload0, stripe_stride, frag_stride, obj, obj_stride, bs, nstripes, stream,
                             obj_size);
}

int xor_decode_join(int k, const std::vector<int>& inputs, const std::vector<int>& outputs,
                    const std::vector<int>& coeff, const void* payload0, int64_t stripe_stride, int64_t frag_stride,
                    void* obj, int64_t obj_stride, int64_t bs, int nstripes, void* stream, int64_t obj_size)
{
    int dev = 0;
    int rc = dev_ensure(&dev);
    if (rc) return rc;
    const size_t R = outputs.size(), K = inputs.size();
    if (R == 0 || K == 0 || coeff.size() != R * K) return dev_fail(ECAMD_EINVAL, "xor decode-join: bad matrix");
    for (int o : outputs)
        if (o < 0 || o >= k) return dev_fail(ECAMD_EINVAL, "xor decode-join: outputs must be data fragments");

    std::shared_ptr<RsEntry> e;  // cached like the RS maps: the map's coefficient tables live on the device
    if ((rc = xor_join_entry(dev, k, inputs, outputs, coeff, e))) return rc;
    return decode_join_entry(*e, k, payload0, stripe_stride, frag_stride, obj, obj_stride, bs, nstripes, stream,
                             obj_size);
}

int crc_encode_prebuild(int k, int m, const uint32_t* masks, int crc_pos, const char* arch, const char* dir)
{
    if (!arch || !dir || k <= 0 || m <= 0 || m > kBsMaxR || k > kBsMaxK) return 0;
    std::vector<int> coeff;
    if (masks) {  // flat XOR: the 0 / 1 matrix of xor_encode_copy_crc_bs
        coeff = xor_coeff(masks, k, m);
    } else {  // rs_vand: the generator's parity rows, as the encode map (m x k)
        FragmentMap fm;
        if (rs_vand_plan(0, k, m, nullptr, -1, 0, fm)) return -1;
        coeff = fm.coeff;
    }
    BsOcc occ{};
    const int prefetch = crc_form_args(m, crc_pos, occ);
    return bitslice_prebuild(coeff, m, k, 0, true, crc_pos, false, nullptr, prefetch, occ, arch, dir);
}

}  // namespace ecamd
