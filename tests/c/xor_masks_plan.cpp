// xor_masks_plan.cpp -- the decode table of ecamd_xor_decode_masks (ecamd_xor_decode_masks_plan, and
// csrc/hip/ecamd_xor_masks_plan.hpp: the entry and the rank xor_decode_masks_kernel runs on the device)
// compiled stand-alone with g++ and compared, for every supported code and every ascending list of fewer
// than hd lost fragments, with what ecamd_xor_plan returns for that list.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ecamd_host.h"
#include "ecamd_xor_masks_plan.hpp"

namespace {

int g_fail = 0;
long g_patterns = 0, g_refused = 0;

struct Code {
    int k, m, hd;
    unsigned int pb[32], db[32];
};

void fail(const Code& c, uint32_t L, const char* what)
{
    if (g_fail++ < 20) std::printf("(%d,%d,%d) mask 0x%08x: %s\n", c.k, c.m, c.hd, L, what);
}

long binom(int n, int t)
{
    long b = 1;
    for (int i = 0; i < t; i++) b = b * (n - i) / (i + 1);
    return b;
}

// f(list, mask) for every ascending list of t of n fragments.
template <class F>
void combinations(int n, int t, F f)
{
    std::vector<int> c(static_cast<size_t>(t));
    for (int i = 0; i < t; i++) c[static_cast<size_t>(i)] = i;
    for (;;) {
        uint32_t L = 0;
        for (int x : c) L |= 1u << x;
        f(c, L);
        int i = t - 1;
        while (i >= 0 && c[static_cast<size_t>(i)] == n - t + i) i--;
        if (i < 0) return;
        c[static_cast<size_t>(i)]++;
        for (int j = i + 1; j < t; j++) c[static_cast<size_t>(j)] = c[static_cast<size_t>(j - 1)] + 1;
    }
}

struct Plan {
    int rc, nout;
    int out[64];
    uint64_t src[64];
};

Plan plan(const Code& c, const std::vector<int>& lost, int decode_parity)
{
    std::vector<int> missing(lost);
    missing.push_back(-1);
    Plan p;
    std::memset(&p, 0, sizeof(p));
    p.nout = -1;
    p.rc = ecamd_xor_plan(1, c.k, c.m, c.hd, c.pb, c.db, missing.data(), decode_parity, p.out, p.src, &p.nout);
    return p;
}

void unrecoverable(const Code& c, uint32_t L)
{
    if (ecamd::xor_masks_rank(c.k + c.m, c.hd, L) != ecamd::kXorMasksUnrecoverable) fail(c, L, "not ranked unrecoverable");
}

void check_code(const Code& c)
{
    const int n = c.k + c.m;
    long want = 0;
    for (int t = 0; t < c.hd; t++) want += binom(n, t);
    const int count = ecamd_xor_decode_masks_plan(c.k, c.m, c.hd, nullptr, 0);
    if (count != want || count != ecamd::xor_masks_count(n, c.hd) || count > ecamd::kXorMasksMaxEntries) {
        fail(c, 0, "entry count is not the sum of C(k+m, t) over t < hd");
        return;
    }
    // one entry more, poisoned: the fill must stop at `count`; and a short capacity must write nothing
    std::vector<ecamd::XorMasksEntry> tab(static_cast<size_t>(count) + 1);
    std::memset(tab.data(), 0xee, tab.size() * sizeof(tab[0]));
    if (ecamd_xor_decode_masks_plan(c.k, c.m, c.hd, tab.data(), count - 1) != count || tab[0].n_out != 0xee)
        fail(c, 0, "a table that is too small was written");
    if (ecamd_xor_decode_masks_plan(c.k, c.m, c.hd, tab.data(), count) != count) fail(c, 0, "fill refused");
    if (tab[static_cast<size_t>(count)].n_out != 0xee) fail(c, 0, "written past the last entry");
    std::vector<char> seen(static_cast<size_t>(count), 0);
    long ranked = 0;
    for (int t = 0; t < c.hd; t++)
        combinations(n, t, [&](const std::vector<int>& lost, uint32_t L) {
            g_patterns++;
            const int32_t rank = ecamd::xor_masks_rank(n, c.hd, L);
            if (rank < 0 || rank >= count || seen[static_cast<size_t>(rank)] || (rank == 0) != (L == 0u)) {
                fail(c, L, "rank out of range, repeated, or 0 for a mask that is not empty");
                return;
            }
            seen[static_cast<size_t>(rank)] = 1;
            ranked++;
            const ecamd::XorMasksEntry& e = tab[static_cast<size_t>(rank)];
            const Plan p1 = plan(c, lost, 1), p0 = plan(c, lost, 0);
            if (p1.rc != 0 || p0.rc != 0) return fail(c, L, "ecamd_xor_plan refuses");
            int ndata = 0;
            for (int f : lost) ndata += f < c.k;
            if (p1.nout != t || p0.nout != ndata || e.n_out != t) return fail(c, L, "output counts differ");
            for (int r = 0; r < ecamd::kXorMasksMaxOut; r++) {
                if (r >= t) {
                    if (e.out[r] != 0 || e.src[r] != 0u) fail(c, L, "unused output not zero");
                    continue;
                }
                const int f = lost[static_cast<size_t>(r)];  // the entry's outputs: the lost fragments ascending
                const int* a1 = std::find(p1.out, p1.out + p1.nout, f);
                if (e.out[r] != f || a1 == p1.out + p1.nout) return fail(c, L, "outputs are not the lost fragments");
                const uint64_t s1 = p1.src[a1 - p1.out];
                // a source names no lost fragment but a lost parity's own slot (the zero-filled accumulator)
                if ((s1 & L & ~(f >= c.k ? 1ull << f : 0ull)) != 0) fail(c, L, "a source names a lost fragment");
                if ((s1 & ~static_cast<uint64_t>(L)) == 0 || (s1 >> n) != 0) fail(c, L, "empty source, or a bit >= k+m");
                if (e.src[r] != (s1 & ~static_cast<uint64_t>(L))) fail(c, L, "source differs from the plan's");
                if (f < c.k) {  // the data rows are the decode_parity 0 plan, unchanged
                    const int* a0 = std::find(p0.out, p0.out + p0.nout, f);
                    if (a0 == p0.out + p0.nout || p0.src[a0 - p0.out] != s1) fail(c, L, "decode_parity 0 row differs");
                    if (r >= ndata) fail(c, L, "a data output behind a parity output");
                }
            }
            uint32_t U = 0;
            for (int r = 0; r < t; r++) U |= e.src[r];
            if (__builtin_popcount(U) > 19) fail(c, L, "more than 19 fragments read");
        });
    if (ranked != count || std::count(seen.begin(), seen.end(), 1) != count) fail(c, 0, "the rank is not onto [0, count)");
    // hd or more bits: the reference refuses the list and touches nothing; the rank says unrecoverable
    combinations(n, c.hd, [&](const std::vector<int>& lost, uint32_t L) {
        g_refused++;
        const Plan p = plan(c, lost, 1);
        if (p.rc != -1 || p.nout != 0) fail(c, L, "a list of hd fragments is not refused");
        unrecoverable(c, L);
    });
    for (int t = c.hd + 1; t <= n; t++) {
        unrecoverable(c, (t < 32 ? 1u << t : 0u) - 1u);           // the lowest t
        unrecoverable(c, ((1u << t) - 1u) << (n - t));            // the highest t
    }
    // a bit >= k+m, alone and beside every recoverable pattern of one fragment
    for (int b = n; b < 32; b++) {
        unrecoverable(c, 1u << b);
        for (int f = 0; f < n; f++) unrecoverable(c, (1u << b) | (1u << f));
    }
    unrecoverable(c, 0xffffffffu);
    unrecoverable(c, 0x80000000u);
}

}  // namespace

int main()
{
    int codes = 0;
    for (int hd = 0; hd <= 6; hd++)
        for (int m = 0; m <= 8; m++)
            for (int k = 0; k <= 32; k++) {
                Code c;
                c.k = k;
                c.m = m;
                c.hd = hd;
                if (k < 1 || m < 1 || ecamd_xor_code_tables(k, m, hd, c.pb, c.db) != 0) {
                    if (ecamd_xor_decode_masks_plan(k, m, hd, nullptr, 0) != -1) fail(c, 0, "a rejected code has a table");
                    continue;
                }
                codes++;
                check_code(c);
            }
    if (codes != 38) {
        std::printf("xor_masks_plan: %d codes, not 38\n", codes);
        g_fail++;
    }
    if (g_patterns != 24229) {
        std::printf("xor_masks_plan: %ld patterns, not 24229\n", g_patterns);
        g_fail++;
    }
    if (g_fail) {
        std::printf("xor_masks_plan: %d mismatches in %ld patterns\n", g_fail, g_patterns);
        return 1;
    }
    std::printf("xor_masks_plan: ok (%d codes, %ld patterns, %ld lists of hd fragments refused)\n", codes, g_patterns, g_refused);
    return 0;
}
