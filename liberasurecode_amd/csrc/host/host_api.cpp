// host_api.cpp -- extern "C" surface of libecamd_host.so (include/ecamd_host.h).
#include "ecamd_host.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bitslice.hpp"
#include "crc.hpp"
#include "ecamd_frame_header.hpp"
#include "ecamd_xor_masks_plan.hpp"
#include "gf16.hpp"
#include "tables.hpp"
#include "xor_plan.hpp"

using namespace ecamd;

namespace {
std::vector<int> minus1_list(const int* missing)
{
    std::vector<int> v;
    if (!missing) return v;
    for (int i = 0; missing[i] > -1; i++) v.push_back(missing[i]);
    return v;
}
}  // namespace

extern "C" {

int ecamd_gf16_mul(int a, int b) { return GF16::get().mul(a & 0xffff, b & 0xffff); }

int ecamd_gf16_inv(int a) { return GF16::get().inv(a & 0xffff); }

int ecamd_rs_generator(int k, int m, int* out)
{
    std::vector<int> g = rs_generator(k, m);
    if (g.empty() || !out) return -1;
    std::memcpy(out, g.data(), g.size() * sizeof(int));
    return 0;
}

int ecamd_gf16_invert(const int* a, int* inv, int n)
{
    if (!a || !inv || n <= 0) return -1;
    std::vector<int> m(a, a + static_cast<size_t>(n) * n), r;
    if (!gf16_invert(m, r, n)) return -1;
    std::memcpy(inv, r.data(), r.size() * sizeof(int));
    return 0;
}

int ecamd_rs_decode_map(const int* G, int k, int m, const int* missing, int rebuild_parity,
                        int* inputs, int* outputs, int* coeff, int* nout)
{
    if (!G || k <= 0 || m < 0) return -1;
    std::vector<int> g(G, G + static_cast<size_t>(k + m) * k);
    FragmentMap fm;
    if (rs_decode_map(g, k, m, minus1_list(missing), rebuild_parity != 0, fm) != 0) return -1;
    std::memcpy(inputs, fm.inputs.data(), fm.inputs.size() * sizeof(int));
    if (!fm.outputs.empty()) {
        std::memcpy(outputs, fm.outputs.data(), fm.outputs.size() * sizeof(int));
        std::memcpy(coeff, fm.coeff.data(), fm.coeff.size() * sizeof(int));
    }
    *nout = static_cast<int>(fm.outputs.size());
    return 0;
}

int ecamd_rs_reconstruct_map(const int* G, int k, int m, const int* missing, int dest, int* inputs,
                             int* ninputs, int* coeff)
{
    if (!G || k <= 0 || m < 0) return -1;
    std::vector<int> g(G, G + static_cast<size_t>(k + m) * k);
    FragmentMap fm;
    if (rs_reconstruct_map(g, k, m, minus1_list(missing), dest, fm) != 0) return -1;
    if (!fm.inputs.empty()) {
        std::memcpy(inputs, fm.inputs.data(), fm.inputs.size() * sizeof(int));
        std::memcpy(coeff, fm.coeff.data(), fm.coeff.size() * sizeof(int));
    }
    *ninputs = static_cast<int>(fm.inputs.size());
    return 0;
}

int ecamd_rs_check_map(const int* G, int k, int m, const int* missing, int* inputs, int* checked,
                       int* coeff, int* ncheck)
{
    if (!G || k <= 0 || m < 0 || !inputs || !ncheck) return -1;
    std::vector<int> g(G, G + static_cast<size_t>(k + m) * k);
    FragmentMap fm;
    if (rs_check_map(g, k, m, minus1_list(missing), fm) != 0) return -1;
    std::memcpy(inputs, fm.inputs.data(), fm.inputs.size() * sizeof(int));
    if (!fm.outputs.empty()) {
        if (!checked || !coeff) return -1;
        std::memcpy(checked, fm.outputs.data(), fm.outputs.size() * sizeof(int));
        std::memcpy(coeff, fm.coeff.data(), fm.coeff.size() * sizeof(int));
    }
    *ncheck = static_cast<int>(fm.outputs.size());
    return 0;
}

int ecamd_rs_locate_map(const int* G, int k, int m, const int* missing, int* inputs, int* checked,
                        int* coeff, int* ncheck, int* ratio)
{
    if (!G || k <= 0 || m < 0 || !inputs || !ncheck) return -1;
    std::vector<int> g(G, G + static_cast<size_t>(k + m) * k);
    FragmentMap fm;
    std::vector<int> rt;
    if (rs_locate_map(g, k, m, minus1_list(missing), fm, rt) != 0) return -1;
    std::memcpy(inputs, fm.inputs.data(), fm.inputs.size() * sizeof(int));
    if (!fm.outputs.empty()) {
        if (!checked || !coeff) return -1;
        std::memcpy(checked, fm.outputs.data(), fm.outputs.size() * sizeof(int));
        std::memcpy(coeff, fm.coeff.data(), fm.coeff.size() * sizeof(int));
    }
    if (!rt.empty()) {
        if (!ratio) return -1;
        std::memcpy(ratio, rt.data(), rt.size() * sizeof(int));
    }
    *ncheck = static_cast<int>(fm.outputs.size());
    return 0;
}

int ecamd_rs_locate_pairs_map(const int* G, int k, int m, const int* missing, int* inputs, int* checked,
                              int* coeff, int* ncheck, int* npairs, int* pivots, int* L, int* independent4)
{
    if (!G || k <= 0 || m < 0 || !inputs || !ncheck || !npairs || !independent4) return -1;
    std::vector<int> g(G, G + static_cast<size_t>(k + m) * k);
    FragmentMap fm;
    if (rs_check_map(g, k, m, minus1_list(missing), fm) != 0) return -1;
    std::memcpy(inputs, fm.inputs.data(), fm.inputs.size() * sizeof(int));
    if (!fm.outputs.empty()) {
        if (!checked || !coeff) return -1;
        std::memcpy(checked, fm.outputs.data(), fm.outputs.size() * sizeof(int));
        std::memcpy(coeff, fm.coeff.data(), fm.coeff.size() * sizeof(int));
    }
    const int R = static_cast<int>(fm.outputs.size());
    const PairPlan plan = rs_locate_pairs_plan(fm.coeff, R, k);
    if (plan.pairs) {
        if (!pivots || !L) return -1;
        std::memcpy(pivots, plan.pivot.data(), plan.pivot.size() * sizeof(int));
        std::memcpy(L, plan.L.data(), plan.L.size() * sizeof(int));
    }
    *ncheck = R;
    *npairs = plan.pairs;
    *independent4 = plan.independent4 ? 1 : 0;
    return 0;
}

int ecamd_rs_correct_map(const int* G, int k, int m, const int* missing, int* inputs, int* checked, int* coeff,
                         int* ncheck, int* pivot, int* scale, int* npairs, int* pair_pivots, int* minv)
{
    if (!G || k <= 0 || m < 0 || !inputs || !ncheck || !pivot || !scale) return -1;
    std::vector<int> g(G, G + static_cast<size_t>(k + m) * k);
    FragmentMap fm;
    if (rs_check_map(g, k, m, minus1_list(missing), fm) != 0) return -1;
    std::memcpy(inputs, fm.inputs.data(), fm.inputs.size() * sizeof(int));
    if (!fm.outputs.empty()) {
        if (!checked || !coeff) return -1;
        std::memcpy(checked, fm.outputs.data(), fm.outputs.size() * sizeof(int));
        std::memcpy(coeff, fm.coeff.data(), fm.coeff.size() * sizeof(int));
    }
    const int R = static_cast<int>(fm.outputs.size());
    const CorrectPlan plan = rs_correct_plan(fm.coeff, R, k);
    std::memcpy(pivot, plan.pivot.data(), plan.pivot.size() * sizeof(int));
    std::memcpy(scale, plan.scale.data(), plan.scale.size() * sizeof(int));
    if (pair_pivots && plan.pairs) std::memcpy(pair_pivots, plan.pair_pivot.data(), plan.pair_pivot.size() * sizeof(int));
    if (minv && plan.pairs) std::memcpy(minv, plan.minv.data(), plan.minv.size() * sizeof(int));
    *ncheck = R;
    if (npairs) *npairs = plan.pairs;
    return 0;
}

int ecamd_split_tables(const int* coeff, int R, int K, int row0, int width, int col0, int ncols,
                       uint8_t* out)
{
    if (!coeff || !out || (width != 2 && width != 4 && width != 8)) return -1;
    std::vector<int> c(coeff, coeff + static_cast<size_t>(R) * K);
    std::vector<uint8_t> img = build_split_tables(c, R, K, row0, width, col0, ncols);
    std::memcpy(out, img.data(), img.size());
    return static_cast<int>(img.size());
}

int ecamd_xor_code_tables(int k, int m, int hd, unsigned int* parity_bms, unsigned int* data_bms)
{
    XorCode c;
    if (!xor_code_lookup(k, m, hd, c)) return -1;
    if (parity_bms) std::memcpy(parity_bms, c.parity_bms, sizeof(unsigned int) * m);
    if (data_bms) std::memcpy(data_bms, c.data_bms, sizeof(unsigned int) * k);
    return 0;
}

int ecamd_xor_check_plan(int k, int m, int hd, unsigned int* sig)
{
    XorCode c;
    if (!sig || !xor_code_lookup(k, m, hd, c)) return -1;
    for (int j = 0; j < k; j++) {
        sig[j] = 0;
        for (int p = 0; p < m; p++)
            if ((c.parity_bms[p] >> j) & 1u) sig[j] |= 1u << p;
    }
    for (int p = 0; p < m; p++) sig[k + p] = 1u << p;
    return 0;
}

int ecamd_xor_check_plan_degraded(int k, int m, int hd, const int* missing, unsigned int* rows, unsigned int* sig,
                                  unsigned int* covered)
{
    XorCode c;
    if (!rows || !sig || !xor_code_lookup(k, m, hd, c)) return -1;
    const int n = k + m;
    unsigned int lost = 0;
    if (missing)
        for (int i = 0; missing[i] > -1; i++) {
            const int f = missing[i];
            if (i >= m || f >= n || ((lost >> f) & 1u)) return -1;
            lost |= 1u << f;
        }
    unsigned int h[32], live = (1u << m) - 1u;
    for (int p = 0; p < m; p++) h[p] = c.parity_bms[p] | 1u << (k + p);
    for (int f = 0; f < n; f++) {  // ascending, whatever the order of the list
        if (!((lost >> f) & 1u)) continue;
        int pv = -1;
        for (int p = 0; p < m && pv < 0; p++)
            if (((live >> p) & 1u) && ((h[p] >> f) & 1u)) pv = p;
        if (pv < 0) continue;
        for (int p = 0; p < m; p++)
            if (p != pv && ((live >> p) & 1u) && ((h[p] >> f) & 1u)) h[p] ^= h[pv];
        live &= ~(1u << pv);
    }
    int alive = 0;
    for (int p = 0; p < m; p++) {
        rows[p] = ((live >> p) & 1u) ? h[p] : 0u;
        alive += static_cast<int>((live >> p) & 1u);
    }
    unsigned int cov = 0;
    for (int f = 0; f < n; f++) {
        sig[f] = 0;
        for (int p = 0; p < m; p++)
            if ((rows[p] >> f) & 1u) sig[f] |= 1u << p;
        if (sig[f]) cov |= 1u << f;
    }
    if (covered) *covered = cov;
    return alive;
}

int ecamd_xor_plan(int op, int k, int m, int hd, const unsigned int* parity_bms,
                   const unsigned int* data_bms, const int* missing, int arg, int* outputs,
                   uint64_t* sources, int* nout)
{
    XorCode c;
    c.k = k;
    c.m = m;
    c.hd = hd;
    c.parity_bms = parity_bms;
    c.data_bms = data_bms;
    if (!parity_bms || !data_bms || k <= 0 || m <= 0 || k + m > 63 || !nout) return -100;
    XorPlan p;
    if (op == 0)
        p = xor_plan_encode(c);
    else if (op == 1)
        p = xor_plan_decode(c, minus1_list(missing), arg);
    else
        p = xor_plan_reconstruct_one(c, minus1_list(missing), arg);
    for (size_t i = 0; i < p.outputs.size(); i++) {
        outputs[i] = p.outputs[i];
        sources[i] = p.sources[i];
    }
    *nout = static_cast<int>(p.outputs.size());
    return p.rc;
}

int ecamd_xor_decode_masks_plan(int k, int m, int hd, void* table, int capacity)
{
    XorCode c;
    if (k <= 0 || m <= 0 || !xor_code_lookup(k, m, hd, c)) return -1;
    const int n = k + m;
    if (n > 32 || hd - 1 > kXorMasksMaxOut) return -2;
    const int count = xor_masks_count(n, hd);
    if (!table || capacity < count) return count;
    auto* tab = static_cast<XorMasksEntry*>(table);
    std::memset(tab, 0, sizeof(XorMasksEntry) * static_cast<size_t>(count));
    for (int t = 0; t < hd; t++) {  // every ascending list of t fragments, in lexicographic order
        std::vector<int> lost(static_cast<size_t>(t));
        for (int i = 0; i < t; i++) lost[i] = i;
        for (;;) {
            uint32_t L = 0;
            for (int f : lost) L |= 1u << f;
            const XorPlan p = xor_plan_decode(c, lost, 1);
            const int32_t rank = xor_masks_rank(n, hd, L);
            if (p.rc != 0 || p.outputs.size() != lost.size() || rank < 0 || rank >= count) return -2;
            XorMasksEntry& e = tab[rank];
            for (int r = 0; r < t; r++) {  // the outputs ascending, whatever the plan's order
                const auto at = std::find(p.outputs.begin(), p.outputs.end(), lost[r]);
                if (at == p.outputs.end()) return -2;
                const uint64_t src = p.sources[static_cast<size_t>(at - p.outputs.begin())] & ~static_cast<uint64_t>(L);
                if (src == 0 || (src >> n) != 0) return -2;
                e.out[r] = static_cast<uint8_t>(lost[r]);
                e.src[r] = static_cast<uint32_t>(src);
            }
            e.n_out = static_cast<uint8_t>(t);
            int i = t - 1;
            while (i >= 0 && lost[i] == n - t + i) i--;
            if (i < 0) break;
            lost[i]++;
            for (int j = i + 1; j < t; j++) lost[j] = lost[j - 1] + 1;
        }
    }
    return count;
}

int ecamd_frame_header(int idx, uint32_t blocksize, uint64_t obj_size, int backend, int checksum, uint32_t payload_crc,
                       int legacy, uint8_t out[80])
{
    if (!out || idx < 0) return -1;
    const CrcMachine mach(legacy != 0);
    uint32_t w[kHeaderWords];
    frame_header_fill(w, frame_header_args(backend, checksum, blocksize, obj_size, 0), static_cast<uint32_t>(idx), payload_crc,
                      mach.t, legacy ? 1 : 0);
    for (int i = 0; i < kHeaderBytes; i++) out[i] = static_cast<uint8_t>(frame_byte(w, i));
    return 0;
}

int ecamd_xor_fragments_needed(int k, int m, int hd, const unsigned int* parity_bms,
                               const unsigned int* data_bms, const int* to_reconstruct,
                               const int* to_exclude, int* needed)
{
    XorCode c;
    c.k = k;
    c.m = m;
    c.hd = hd;
    c.parity_bms = parity_bms;
    c.data_bms = data_bms;
    std::vector<int> out;
    int rc = xor_fragments_needed(c, minus1_list(to_reconstruct), minus1_list(to_exclude), out);
    if (rc >= 0 && needed) std::memcpy(needed, out.data(), out.size() * sizeof(int));
    return rc;
}

int ecamd_fragments_needed_batch(int backend, int k, int m, int hd, const int* recon,
                                 const int* excl, int list_stride, int nstripes, int* needed,
                                 int* rcs)
{
    if (!recon || !excl || !needed || !rcs || list_stride < 1 || nstripes < 0 || k < 1 || m < 0 ||
        k + m > 64)
        return -1;
    unsigned pb[64], db[64];
    if (backend == 3 && ecamd_xor_code_tables(k, m, hd, pb, db) != 0) return -1;
    if (backend != 3 && backend != 6) return -1;
    const int row = k + m + 1;
    for (int s = 0; s < nstripes; s++) {
        const int* r = recon + static_cast<int64_t>(s) * list_stride;
        const int* x = excl + static_cast<int64_t>(s) * list_stride;
        int* out = needed + static_cast<int64_t>(s) * row;
        std::vector<int> rl, xl;
        for (int i = 0; i < list_stride && r[i] >= 0; i++) rl.push_back(r[i]);
        for (int i = 0; i < list_stride && x[i] >= 0; i++) xl.push_back(x[i]);
        rl.push_back(-1);
        xl.push_back(-1);
        if (backend == 3) {
            // xor_hd_fragments_needed (xor_hd_code.c:209-412), exactly as the shim calls it
            std::vector<int> tmp(row, -1);
            rcs[s] = ecamd_xor_fragments_needed(k, m, hd, pb, db, rl.data(), xl.data(), tmp.data());
            std::memcpy(out, tmp.data(), sizeof(int) * row);
            if (rcs[s] >= 0) {
                int n = 0;
                while (n < row && tmp[n] >= 0) n++;
                for (int i = n; i < row; i++) out[i] = -1;
            }
        } else {
            // rs_vand shim (src/backends/rs_vand/liberasurecode_rs_vand.c:119-145): the first k
            // indices neither missing nor excluded.
            std::vector<bool> gone(k + m, false);
            for (int v : xl)
                if (v >= 0 && v < k + m) gone[v] = true;
            for (int v : rl)
                if (v >= 0 && v < k + m) gone[v] = true;
            int j = 0;
            for (int i = 0; i < k + m && j < k; i++)
                if (!gone[i]) out[j++] = i;
            for (int i = j; i < row; i++) out[i] = -1;
            rcs[s] = j == k ? 0 : -1;
        }
    }
    return 0;
}

int ecamd_percall_device_plan(int ndev, const char* spec, int* devs, int max)
{
    if (ndev <= 0 || !devs || max <= 0) return 0;
    std::vector<int> ids;
    std::vector<bool> seen(static_cast<size_t>(ndev), false);
    for (const char* p = spec; p && *p;) {
        char* end = nullptr;
        const long v = std::strtol(p, &end, 10);
        if (end == p) {  // not a number: skip one character (separators, spaces)
            p++;
            continue;
        }
        if (v >= 0 && v < ndev && !seen[static_cast<size_t>(v)]) {
            seen[static_cast<size_t>(v)] = true;
            ids.push_back(static_cast<int>(v));
        }
        p = end;
    }
    if (ids.empty())
        for (int d = 0; d < ndev; d++) ids.push_back(d);
    const int n = std::min(static_cast<int>(ids.size()), max);
    for (int i = 0; i < n; i++) devs[i] = ids[static_cast<size_t>(i)];
    return n;
}

int ecamd_bitslice_eval(const int* coeff, int R, int K, int cap, const uint16_t* in, uint16_t* out,
                        int* ops)
{
    if (!coeff || !in || !out || R <= 0 || R > kBsMaxR || K <= 0 || K > kBsMaxK) return -1;
    std::vector<int> c(coeff, coeff + static_cast<size_t>(R) * K);
    const BitsliceNet net = bitslice_network(c, R, K, cap);
    bitslice_eval(net, in, out);
    if (ops) *ops = net.xor_ops();
    return 0;
}

int64_t ecamd_bitslice_source(const int* coeff, int R, int K, int cap, int depth, char* buf, int64_t size)
{
    if (!coeff || R <= 0 || R > kBsMaxR || K <= 0 || K > kBsMaxK) return -1;
    std::vector<int> c(coeff, coeff + static_cast<size_t>(R) * K);
    const std::string src = bitslice_source(bitslice_network(c, R, K, cap), depth);
    if (buf && size > 0) {
        const size_t n = std::min(static_cast<size_t>(size - 1), src.size());
        std::memcpy(buf, src.data(), n);
        buf[n] = 0;
    }
    return static_cast<int64_t>(src.size());
}

namespace {
int64_t copy_out(const std::string& text, char* buf, int64_t size)
{
    if (buf && size > 0) {
        const size_t n = std::min(static_cast<size_t>(size - 1), text.size());
        std::memcpy(buf, text.data(), n);
        buf[n] = 0;
    }
    return static_cast<int64_t>(text.size());
}
}  // namespace

int64_t ecamd_bitslice_wave_request(const int* coeff, int R, int K, int cap, int opts, char* buf, int64_t size)
{
    if (!coeff || R <= 0 || R > kBsMaxR || K <= 0 || K > kBsMaxK) return -1;
    const std::vector<int> c(coeff, coeff + static_cast<size_t>(R) * K);
    BsOcc occ;
    occ.barrier = true;
    return copy_out(bitslice_request(c, R, K, cap, 0, false, false, 1, false, false, true, nullptr, 0, &occ, 0, false,
                                     false, opts),
                    buf, size);
}

int ecamd_bitslice_request_opts(const char* request)
{
    std::vector<int> c;
    int R = 0, K = 0, cap = 0, depth = 0;
    BitsliceStyle style;
    if (!request || !bitslice_request_style(request, c, R, K, cap, depth, style)) return -1;
    return style.opts;
}

int64_t ecamd_bitslice_request_source(const char* request, char* buf, int64_t size)
{
    std::vector<int> c;
    int R = 0, K = 0, cap = 0, depth = 0;
    BitsliceStyle style;
    if (!request || !bitslice_request_style(request, c, R, K, cap, depth, style)) return -1;
    return copy_out(bitslice_source(bitslice_network(c, R, K, cap), depth, style), buf, size);
}

}  // extern "C"
