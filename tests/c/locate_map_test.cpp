// Stand-alone host check of ecamd_rs_locate_map (include/ecamd_host.h), built together with the host
// planning sources -- plain and with -fsanitize=address,undefined (tests/test_locate_host.py).  For each
// code and missing pattern: the buffers are exactly as large as the header promises (the sanitizer sees
// any write past them), every entry of the check map is non-zero, ratio[r-1][j] * coeff[0][j] ==
// coeff[r][j], and the rule the ratios serve names every single corrupted fragment of a random word.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ecamd_host.h"

static int fails = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);      \
            fails++;                                                     \
        }                                                                \
    } while (0)

static void one(int k, int m, std::vector<int> missing)
{
    std::vector<int> G(static_cast<size_t>(k + m) * k);
    CHECK(ecamd_rs_generator(k, m, G.data()) == 0);
    const int nmiss = static_cast<int>(missing.size());
    missing.push_back(-1);
    const int R = m - nmiss;
    if (R < 0) {
        std::vector<int> inputs(static_cast<size_t>(k));
        int n = -7;
        CHECK(ecamd_rs_locate_map(G.data(), k, m, missing.data(), inputs.data(), nullptr, nullptr, &n, nullptr) == -1);
        return;
    }
    std::vector<int> inputs(static_cast<size_t>(k)), checked(static_cast<size_t>(R)), coeff(static_cast<size_t>(R) * k),
        ratio(static_cast<size_t>(R > 1 ? R - 1 : 0) * k);
    int n = -7;
    CHECK(ecamd_rs_locate_map(G.data(), k, m, missing.data(), inputs.data(), R ? checked.data() : nullptr,
                              R ? coeff.data() : nullptr, &n, ratio.empty() ? nullptr : ratio.data()) == 0);
    CHECK(n == R);
    for (int c : coeff) CHECK(c > 0 && c <= 0xffff);
    for (int r = 1; r < R; r++)
        for (int j = 0; j < k; j++)
            CHECK(ecamd_gf16_mul(ratio[static_cast<size_t>(r - 1) * k + j], coeff[static_cast<size_t>(j)]) ==
                  coeff[static_cast<size_t>(r) * k + j]);
    if (R < 2) return;
    // the rule on one word: error e in participant c (inputs 0..k-1, then the checked rows)
    unsigned seed = 12345u + static_cast<unsigned>(k * 64 + m);
    for (int c = 0; c < k + R; c++) {
        seed = seed * 1664525u + 1013904223u;
        const int e = static_cast<int>(seed >> 16) | 1;
        std::vector<int> S(static_cast<size_t>(R), 0);
        for (int r = 0; r < R; r++) S[static_cast<size_t>(r)] = c < k ? ecamd_gf16_mul(coeff[static_cast<size_t>(r) * k + c], e) : (r == c - k ? e : 0);
        int found = 0, who = -1;
        for (int j = 0; j < k; j++) {
            bool ok = true;
            for (int r = 1; r < R; r++)
                ok = ok && S[static_cast<size_t>(r)] == ecamd_gf16_mul(ratio[static_cast<size_t>(r - 1) * k + j], S[0]);
            if (ok) found++, who = j;
        }
        for (int q = 0; q < R; q++) {
            bool ok = true;
            for (int r = 0; r < R; r++) ok = ok && (r == q || S[static_cast<size_t>(r)] == 0);
            if (ok) found++, who = k + q;
        }
        CHECK(found == 1 && who == c);
    }
}

int main()
{
    const int codes[][2] = {{10, 4}, {4, 2}, {20, 8}, {3, 1}, {1, 3}};
    for (const auto& c : codes) {
        const int k = c[0], m = c[1], n = k + m;
        one(k, m, {});
        one(k, m, {0});
        one(k, m, {n - 1});
        if (m >= 2) one(k, m, {n > 7 ? 2 : 0, n > 7 ? 7 : 1});
        std::vector<int> all;
        for (int i = 0; i < m; i++) all.push_back(i);
        one(k, m, all);
        all.push_back(m);
        one(k, m, all);
    }
    if (fails) return 1;
    std::printf("locate_map: ok\n");
    return 0;
}
