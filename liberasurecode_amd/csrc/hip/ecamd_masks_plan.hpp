// ecamd_masks_plan.hpp -- the per-stripe plan of ecamd_rs_decode_masks: from the generator of the
// rs_vand code (k, m) and the mask of one stripe's lost fragments, the record decode_masks_kernel
// consumes -- which k fragments to read, which to write, with which coefficients (DESIGN.md "Decode
// from device masks").  Written once: plain C++ that masks_plan_kernel runs on the device, the 64
// lanes of a wave sharing one stripe, and tests/c/masks_plan.cpp runs on the host as a single lane
// against ecamd_rs_decode_map, whose record it must equal entry for entry (the inverse is unique, so
// there is nothing to tolerate).
//
// Field arithmetic is shift and xor over 0x1100b; there are no log tables (128 KiB per table: they
// do not fit the LDS, and a lane-private walk through them in global memory is what the plan avoids).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define ECAMD_MASKS_HD __host__ __device__ __forceinline__
#else
#define ECAMD_MASKS_HD inline
#endif

namespace ecamd {

constexpr int kMasksMaxFrags = 32;  // k + m: one mask word per stripe
constexpr int kMasksMaxOut = 8;     // m: fragments rebuilt per stripe, rows of the widest table entry

// What one stripe's workgroups read.  result is the stripe's d_result word: 0 for an empty mask, the
// number of fragments rebuilt (n_out), or 0x80000000 | popcount for an unrecoverable mask (n_out 0).
// in[j], j < k: the first k fragments not lost.  out[r], r < n_out: the lost data fragments ascending,
// then -- with rebuild_parity -- the lost parity fragments ascending.  coef[r*k + j]: output r =
// sum_j coef[r*k + j] * input j.  560 bytes, a multiple of 16.
struct MasksRecord {
    uint32_t n_out;
    uint32_t result;
    uint8_t in[kMasksMaxFrags];
    uint8_t out[kMasksMaxOut];
    uint16_t coef[kMasksMaxOut * kMasksMaxFrags];
};
static_assert(sizeof(MasksRecord) == 560, "MasksRecord layout");

// Scratch of one plan, shared by its lanes (LDS on the device): the t x t minor M and its inverse V in
// rows of kMasksMaxOut, the pivot column, the input and output indices, and the rows of the lost data.
struct MasksPlanWork {
    uint16_t M[kMasksMaxOut * kMasksMaxOut];
    uint16_t V[kMasksMaxOut * kMasksMaxOut];
    uint16_t col[kMasksMaxOut];
    uint16_t in[kMasksMaxFrags];
    uint16_t out[kMasksMaxOut];
    uint16_t rows[kMasksMaxOut * kMasksMaxFrags];
};

// c times both 16-bit words of x in GF(2^16), polynomial 0x1100b (gf16_mul2 of ecamd_check.hip).
ECAMD_MASKS_HD uint32_t masks_gf_mul2(uint32_t c, uint32_t x)
{
    uint32_t acc = 0;
    for (int b = 0; b < 16; b++) {
        if ((c >> b) & 1u) acc ^= x;
        const uint32_t hi = x & 0x80008000u;
        x = ((x & 0x7fff7fffu) << 1) ^ ((hi >> 15) * 0x100bu);
    }
    return acc;
}

ECAMD_MASKS_HD uint32_t masks_gf_mul(uint32_t a, uint32_t b) { return masks_gf_mul2(a, b & 0xffffu) & 0xffffu; }

// a^(2^16 - 2): the product of a^(2^i), i = 1..15.
ECAMD_MASKS_HD uint32_t masks_gf_inv(uint32_t a)
{
    uint32_t p = masks_gf_mul(a, a), r = p;
    for (int i = 2; i < 16; i++) {
        p = masks_gf_mul(p, p);
        r = masks_gf_mul(r, p);
    }
    return r;
}

ECAMD_MASKS_HD int masks_popcount(uint32_t v)
{
    int n = 0;
    for (; v; v &= v - 1) n++;
    return n;
}

ECAMD_MASKS_HD uint32_t masks_below(int f) { return f < 32 ? (1u << f) - 1u : 0xffffffffu; }

// The record of mask L over the generator G ((k+m) x k, row-major: ecamd_rs_generator's entries as
// 16-bit words); k >= 1, k + m <= 32, m <= 8.  Returns the stripe's result word (rec->result).
//
// With t lost data fragments, P the first t surviving parities and M = G[P][lost data] (t x t):
//   lost data a      = sum_i inv(M)[a][i] * (P_i ^ sum_s G[P_i][s] * s), s over the surviving data,
//   lost parity q    = sum_s G[q][s] * s ^ sum_a G[q][lost a] * (lost data a),
// which over the inputs (surviving data, then P) are the rows written below.
//
// `nlanes` lanes work on one plan, this one being `lane`: every loop over independent elements is
// strided over them, and sync() stands between a step's stores to *w / *rec and the next step's loads
// (a workgroup barrier on the device; the host runs one lane with a sync that does nothing).  Every lane
// takes the same branches -- they depend only on L, G and what all lanes read from *w -- so every lane
// reaches every sync(), and every lane returns the result.
template <class Sync>
ECAMD_MASKS_HD uint32_t masks_plan(const uint16_t* G, int k, int m, uint32_t L, int rebuild_parity, MasksRecord* rec,
                                   MasksPlanWork* w, int lane, int nlanes, Sync sync)
{
    const int n = k + m;
    const int lost = masks_popcount(L);
    uint32_t result = 0u;
    if (L != 0u && ((L & ~masks_below(n)) != 0u || lost > m)) result = 0x80000000u | static_cast<uint32_t>(lost);
    if (L == 0u || result != 0u) {
        if (lane == 0) {
            rec->n_out = 0u;
            rec->result = result;
        }
        return result;
    }
    const int t = masks_popcount(L & masks_below(k)), nsd = k - t;
    const int np = rebuild_parity ? lost - t : 0, no = t + np;
    // inputs: the surviving data, then the first t surviving parities; outputs: the lost data, then the
    // lost parities.  A fragment's place is the number of its kind below it.
    for (int f = lane; f < n; f += nlanes) {
        if (!((L >> f) & 1u)) {
            const int at = masks_popcount(~L & masks_below(f));
            if (at < k) {
                w->in[at] = static_cast<uint16_t>(f);
                rec->in[at] = static_cast<uint8_t>(f);
            }
        } else if (f < k || rebuild_parity) {
            const int at = masks_popcount(L & masks_below(f));  // the lost data come first: all of them are below k
            w->out[at] = static_cast<uint16_t>(f);
            rec->out[at] = static_cast<uint8_t>(f);
        }
    }
    sync();
    constexpr int P = kMasksMaxOut;
    for (int e = lane; e < t * t; e += nlanes) {
        const int i = e / t, a = e - i * t;
        w->M[i * P + a] = G[w->in[nsd + i] * k + w->out[a]];
        w->V[i * P + a] = i == a ? 1 : 0;
    }
    sync();
    // Gauss-Jordan: [M | I] -> [I | inv(M)]; any t x t minor of the parity rows is non-singular
    for (int i = 0; i < t; i++) {
        int pr = i;
        while (pr < t && w->M[pr * P + i] == 0) pr++;
        if (pr == t) {  // (never: the code is MDS)
            if (lane == 0) {
                rec->n_out = 0u;
                rec->result = 0x80000000u | static_cast<uint32_t>(lost);
            }
            return 0x80000000u | static_cast<uint32_t>(lost);
        }
        sync();
        if (pr != i) {
            for (int e = lane; e < 2 * t; e += nlanes) {
                uint16_t* a = e < t ? w->M : w->V;
                const int c = e < t ? e : e - t;
                const uint16_t x = a[pr * P + c];
                a[pr * P + c] = a[i * P + c];
                a[i * P + c] = x;
            }
            sync();
        }
        for (int r = lane; r < t; r += nlanes) w->col[r] = w->M[r * P + i];
        sync();
        const uint32_t d = w->col[i];
        if (d != 1u) {
            const uint32_t f = masks_gf_inv(d);
            for (int e = lane; e < 2 * t; e += nlanes) {
                uint16_t* a = e < t ? w->M : w->V;
                const int c = e < t ? e : e - t;
                a[i * P + c] = static_cast<uint16_t>(masks_gf_mul(f, a[i * P + c]));
            }
            sync();
        }
        for (int e = lane; e < t * 2 * t; e += nlanes) {
            const int r = e / (2 * t), cc = e - r * 2 * t;
            const uint32_t f = w->col[r];
            if (r == i || f == 0u) continue;
            uint16_t* a = cc < t ? w->M : w->V;
            const int c = cc < t ? cc : cc - t;
            a[r * P + c] ^= static_cast<uint16_t>(masks_gf_mul(f, a[i * P + c]));
        }
        sync();
    }
    // rows of the lost data: inv(M) times [G[P][surviving data] | I]
    for (int e = lane; e < t * k; e += nlanes) {
        const int a = e / k, j = e - a * k;
        uint32_t c = 0;
        if (j < nsd)
            for (int i = 0; i < t; i++) c ^= masks_gf_mul(w->V[a * P + i], G[w->in[nsd + i] * k + w->in[j]]);
        else
            c = w->V[a * P + (j - nsd)];
        w->rows[e] = static_cast<uint16_t>(c);
        rec->coef[e] = static_cast<uint16_t>(c);
    }
    sync();
    // rows of the lost parities: G[q] times those rows, with unit rows for the surviving data
    for (int e = lane; e < np * k; e += nlanes) {
        const int r = t + e / k, j = e - (r - t) * k, q = w->out[r];
        uint32_t c = j < nsd ? G[q * k + w->in[j]] : 0u;
        for (int a = 0; a < t; a++) c ^= masks_gf_mul(G[q * k + w->out[a]], w->rows[a * k + j]);
        rec->coef[r * k + j] = static_cast<uint16_t>(c);
    }
    if (lane == 0) {
        rec->n_out = static_cast<uint32_t>(no);
        rec->result = static_cast<uint32_t>(no);
    }
    return static_cast<uint32_t>(no);
}

}  // namespace ecamd
