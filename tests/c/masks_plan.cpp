// masks_plan.cpp -- the per-stripe plan of ecamd_rs_decode_masks (csrc/hip/ecamd_masks_plan.hpp, the
// text masks_plan_kernel runs on the device) compiled stand-alone with g++ and compared, entry for
// entry, with what ecamd_rs_decode_map returns for the ascending list of the same mask: the same
// inputs, the same outputs, the same coefficients, for both values of rebuild_parity.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ecamd_host.h"
#include "ecamd_masks_plan.hpp"

namespace {

int g_fail = 0;
long g_cases = 0;

uint64_t splitmix(uint64_t& s)
{
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

struct Code {
    int k, m;
    std::vector<int> G;
    std::vector<uint16_t> G16;
    Code(int k_, int m_) : k(k_), m(m_), G(static_cast<size_t>(k_ + m_) * k_)
    {
        if (ecamd_rs_generator(k, m, G.data()) != 0) {
            std::printf("no generator for (%d,%d)\n", k, m);
            g_fail++;
        }
        for (int v : G) G16.push_back(static_cast<uint16_t>(v));
    }
};

void fail(const Code& c, uint32_t L, int rp, const char* what)
{
    if (g_fail++ < 20) std::printf("(%d,%d) mask 0x%08x rebuild_parity %d: %s\n", c.k, c.m, L, rp, what);
}

// A recoverable mask: the record against the map.
void compare(const Code& c, uint32_t L)
{
    std::vector<int> missing;
    for (int f = 0; f < c.k + c.m; f++)
        if ((L >> f) & 1u) missing.push_back(f);
    missing.push_back(-1);
    for (int rp = 0; rp < 2; rp++) {
        g_cases++;
        std::vector<int> in(static_cast<size_t>(c.k)), out(32), coef(static_cast<size_t>(32) * c.k);
        int nout = -1;
        if (ecamd_rs_decode_map(c.G.data(), c.k, c.m, missing.data(), rp, in.data(), out.data(), coef.data(), &nout) != 0) {
            fail(c, L, rp, "ecamd_rs_decode_map refuses");
            continue;
        }
        ecamd::MasksRecord rec;
        std::memset(&rec, 0xee, sizeof(rec));
        ecamd::MasksPlanWork work;
        std::memset(&work, 0xdd, sizeof(work));
        const uint32_t res = ecamd::masks_plan(c.G16.data(), c.k, c.m, L, rp, &rec, &work, 0, 1, [] {});
        if (res != static_cast<uint32_t>(nout) || rec.result != res || rec.n_out != res) {
            fail(c, L, rp, "result / n_out differ from the map's output count");
            continue;
        }
        if (L == 0u) continue;  // nothing else of the record is defined
        for (int j = 0; j < c.k; j++)
            if (rec.in[j] != in[static_cast<size_t>(j)]) fail(c, L, rp, "inputs differ");
        for (int r = 0; r < nout; r++) {
            if (rec.out[r] != out[static_cast<size_t>(r)]) fail(c, L, rp, "outputs differ");
            for (int j = 0; j < c.k; j++)
                if (rec.coef[r * c.k + j] != coef[static_cast<size_t>(r) * c.k + j]) fail(c, L, rp, "coefficients differ");
        }
    }
}

void unrecoverable(const Code& c, uint32_t L)
{
    for (int rp = 0; rp < 2; rp++) {
        g_cases++;
        ecamd::MasksRecord rec;
        std::memset(&rec, 0xee, sizeof(rec));
        ecamd::MasksPlanWork work;
        std::memset(&work, 0xdd, sizeof(work));
        const uint32_t res = ecamd::masks_plan(c.G16.data(), c.k, c.m, L, rp, &rec, &work, 0, 1, [] {});
        const uint32_t want = 0x80000000u | static_cast<uint32_t>(__builtin_popcount(L));
        if (res != want || rec.result != want || rec.n_out != 0u) fail(c, L, rp, "not reported unrecoverable");
    }
}

// Every mask over n fragments with at most `most` bits.
void every(const Code& c, int most)
{
    const int n = c.k + c.m;
    for (uint32_t L = 0; L < (1u << n); L++)
        if (__builtin_popcount(L) <= most) compare(c, L);
}

uint32_t random_mask(uint64_t& seed, int n, int bits)
{
    uint32_t L = 0;
    while (__builtin_popcount(L) < bits) L |= 1u << (splitmix(seed) % static_cast<uint64_t>(n));
    return L;
}

}  // namespace

int main()
{
    {
        const Code c(10, 4);
        every(c, 4);  // 1471 patterns
        unrecoverable(c, 0x1fu);
        unrecoverable(c, 1u << 14);
        unrecoverable(c, 0x80000001u);
    }
    {
        const Code c(4, 2);
        every(c, 2);  // 22 patterns
        unrecoverable(c, 0x7u);
        unrecoverable(c, 1u << 6);
    }
    {
        const Code c(20, 8);
        const int n = 28;
        compare(c, 0u);
        for (int a = 0; a < n; a++) {
            compare(c, 1u << a);
            for (int b = a + 1; b < n; b++) compare(c, (1u << a) | (1u << b));
        }
        compare(c, 0xffu);  // the two C5 patterns of prebuild.py
        uint32_t second = 0;
        for (int f : {0, 2, 4, 6, 20, 22, 24, 26}) second |= 1u << f;
        compare(c, second);
        uint64_t seed = 20008;
        for (int i = 0; i < 2000; i++) compare(c, random_mask(seed, n, 3 + static_cast<int>(splitmix(seed) % 6)));
        unrecoverable(c, 0x1ffu);
        unrecoverable(c, 1u << 28);
    }
    {
        const Code c(24, 8);
        uint64_t seed = 24008;
        for (int i = 0; i < 500; i++) compare(c, random_mask(seed, 32, 1 + static_cast<int>(splitmix(seed) % 8)));
        unrecoverable(c, 0x1ffu);  // k + m == 32: no bit is out of range, only the count can be
    }
    if (g_fail) {
        std::printf("masks_plan: %d mismatches in %ld cases\n", g_fail, g_cases);
        return 1;
    }
    std::printf("masks_plan: ok (%ld cases)\n", g_cases);
    return 0;
}
