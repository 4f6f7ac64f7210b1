// gf16.cpp -- see gf16.hpp for the reference mapping.
#include "gf16.hpp"

#include <algorithm>

namespace ecamd {

GF16::GF16() : log_(65536, 0), exp_(2 * kOrder + 2, 0)
{
    // Powers of the generator 2 (x) in the polynomial basis; rs_galois.c:49-71.
    int v = 1;
    for (int e = 0; e < kOrder; e++) {
        log_[v] = e;
        exp_[e] = v;
        exp_[e + kOrder] = v;
        v <<= 1;
        if (v & 0x10000) v ^= kPoly;
    }
}

const GF16& GF16::get()
{
    static const GF16 field;
    return field;
}

namespace {

// Column elimination helpers over a row-major matrix with `cols` columns.
void scale_column(std::vector<int>& a, int cols, int row0, int nrows, int col, int f)
{
    const GF16& gf = GF16::get();
    for (int r = row0; r < row0 + nrows; r++) a[r * cols + col] = gf.mul(a[r * cols + col], f);
}

void add_scaled_column(std::vector<int>& a, int cols, int nrows, int src, int dst, int f)
{
    const GF16& gf = GF16::get();
    for (int r = 0; r < nrows; r++) a[r * cols + dst] ^= gf.mul(a[r * cols + src], f);
}

int pivot_row(const std::vector<int>& a, int cols, int nrows, int col, int from)
{
    for (int r = from; r < nrows; r++)
        if (a[r * cols + col] != 0) return r;
    return -1;
}

void swap_rows(std::vector<int>& a, int cols, int r1, int r2)
{
    for (int c = 0; c < cols; c++) std::swap(a[r1 * cols + c], a[r2 * cols + c]);
}

}  // namespace

std::vector<int> rs_generator(int k, int m)
{
    const GF16& gf = GF16::get();
    const int n = k + m;
    if (k <= 0 || m < 0 || n > 65536) return {};
    std::vector<int> g(static_cast<size_t>(n) * k, 0);
    g[0] = 1;  // evaluation point 0: row e0
    for (int r = 1; r < n; r++) {
        int p = 1;
        for (int c = 0; c < k; c++) {
            g[r * k + c] = p;
            p = gf.mul(p, r);
        }
    }
    // Reduce the top k x k block to the identity by column operations (the code stays MDS).
    for (int d = 1; d < k; d++) {
        int pr = pivot_row(g, k, n, d, d);
        if (pr < 0) return {};
        if (pr != d) swap_rows(g, k, pr, d);
        if (g[d * k + d] != 1) scale_column(g, k, 0, n, d, gf.inv(g[d * k + d]));
        for (int c = 0; c < k; c++) {
            int v = g[d * k + c];
            if (c != d && v != 0) add_scaled_column(g, k, n, d, c, v);
        }
    }
    // First parity row -> all ones (scales only the parity part of each column).
    for (int c = 0; c < k && m > 0; c++) {
        int v = g[k * k + c];
        if (v != 1) scale_column(g, k, k, m, c, gf.inv(v));
    }
    return g;
}

bool gf16_invert(std::vector<int> a, std::vector<int>& inv, int n)
{
    const GF16& gf = GF16::get();
    inv.assign(static_cast<size_t>(n) * n, 0);
    for (int i = 0; i < n; i++) inv[i * n + i] = 1;
    for (int i = 0; i < n; i++) {
        int pr = pivot_row(a, n, n, i, i);
        if (pr < 0) return false;
        if (pr != i) {
            swap_rows(a, n, pr, i);
            swap_rows(inv, n, pr, i);
        }
        int d = a[i * n + i];
        if (d != 1) {
            int f = gf.inv(d);
            for (int c = 0; c < n; c++) {
                a[i * n + c] = gf.mul(a[i * n + c], f);
                inv[i * n + c] = gf.mul(inv[i * n + c], f);
            }
        }
        for (int r = 0; r < n; r++) {
            int f = a[r * n + i];
            if (r == i || f == 0) continue;
            for (int c = 0; c < n; c++) {
                a[r * n + c] ^= gf.mul(a[i * n + c], f);
                inv[r * n + c] ^= gf.mul(inv[i * n + c], f);
            }
        }
    }
    return true;
}

namespace {

struct Availability {
    std::vector<char> missing;   // per fragment index
    std::vector<int> first_k;    // first k present indices, index order
    int nmissing = 0;            // entries in the -1-terminated list (duplicates counted)
};

bool availability(int k, int m, const std::vector<int>& missing, Availability& av)
{
    const int n = k + m;
    av.missing.assign(n, 0);
    av.nmissing = static_cast<int>(missing.size());
    for (int idx : missing)
        if (idx >= 0 && idx < n) av.missing[idx] = 1;
    if (av.nmissing > m) return false;
    for (int i = 0; i < n && static_cast<int>(av.first_k.size()) < k; i++)
        if (!av.missing[i]) av.first_k.push_back(i);
    return static_cast<int>(av.first_k.size()) == k;
}

// Inverse of the decoding matrix built from the generator rows of `first_k`.
bool decode_inverse(const std::vector<int>& G, int k, const std::vector<int>& first_k,
                    std::vector<int>& inv)
{
    std::vector<int> dec(static_cast<size_t>(k) * k);
    for (int r = 0; r < k; r++)
        std::copy(&G[first_k[r] * k], &G[first_k[r] * k] + k, &dec[r * k]);
    return gf16_invert(dec, inv, k);
}

// Coefficients over first_k that rebuild parity fragment `p` (reconstruct's composite row).
std::vector<int> parity_row(const std::vector<int>& G, int k, const Availability& av,
                            const std::vector<int>& missing, const std::vector<int>& inv, int p)
{
    const GF16& gf = GF16::get();
    std::vector<int> row(k, 0);
    int j = 0;
    for (int d = 0; d < k; d++)
        if (!av.missing[d]) row[j++] = G[p * k + d];
    for (int d : missing) {
        if (d < 0 || d >= k) continue;
        for (int c = 0; c < k; c++) row[c] ^= gf.mul(G[p * k + d], inv[d * k + c]);
    }
    return row;
}

// The reference dot product zeroes its output and then accumulates in input order, so an
// input that IS the output reads the partial sum: out <- (1 + c) * out at that step.  Fold
// that into coefficients over the remaining inputs (bit-exact, per 16-bit word).
void fold_alias(std::vector<int>& inputs, std::vector<int>& row, int out_idx)
{
    auto it = std::find(inputs.begin(), inputs.end(), out_idx);
    if (it == inputs.end()) return;
    const GF16& gf = GF16::get();
    std::vector<int> acc(inputs.size(), 0);
    for (size_t i = 0; i < inputs.size(); i++) {
        if (inputs[i] == out_idx) {
            int f = 1 ^ row[i];
            for (auto& v : acc) v = gf.mul(v, f);
        } else {
            acc[i] ^= row[i];
        }
    }
    size_t pos = static_cast<size_t>(it - inputs.begin());
    acc.erase(acc.begin() + pos);
    inputs.erase(inputs.begin() + pos);
    row = acc;
}

}  // namespace

FragmentMap rs_encode_map(const std::vector<int>& G, int k, int m)
{
    FragmentMap fm;
    for (int j = 0; j < k; j++) fm.inputs.push_back(j);
    for (int p = 0; p < m; p++) {
        fm.outputs.push_back(k + p);
        fm.coeff.insert(fm.coeff.end(), &G[(k + p) * k], &G[(k + p) * k] + k);
    }
    return fm;
}

int rs_decode_map(const std::vector<int>& G, int k, int m, const std::vector<int>& missing,
                  bool rebuild_parity, FragmentMap& out)
{
    Availability av;
    if (!availability(k, m, missing, av)) return -1;
    std::vector<int> inv;
    if (!decode_inverse(G, k, av.first_k, inv)) return -1;
    out = FragmentMap();
    out.inputs = av.first_k;
    for (int d = 0; d < k; d++) {
        if (!av.missing[d]) continue;
        out.outputs.push_back(d);
        out.coeff.insert(out.coeff.end(), &inv[d * k], &inv[d * k] + k);
    }
    if (rebuild_parity) {
        for (int p = k; p < k + m; p++) {
            if (!av.missing[p]) continue;
            std::vector<int> row = parity_row(G, k, av, missing, inv, p);
            out.outputs.push_back(p);
            out.coeff.insert(out.coeff.end(), row.begin(), row.end());
        }
    }
    return 0;
}

int rs_reconstruct_map(const std::vector<int>& G, int k, int m, const std::vector<int>& missing,
                       int dest, FragmentMap& out)
{
    Availability av;
    if (dest < 0 || dest >= k + m) return -1;
    if (!availability(k, m, missing, av)) return -1;
    std::vector<int> inv;
    if (!decode_inverse(G, k, av.first_k, inv)) return -1;
    std::vector<int> row;
    if (dest < k)
        row.assign(&inv[dest * k], &inv[dest * k] + k);
    else
        row = parity_row(G, k, av, missing, inv, dest);
    out = FragmentMap();
    out.inputs = av.first_k;
    fold_alias(out.inputs, row, dest);
    out.outputs.push_back(dest);
    out.coeff = row;
    return 0;
}

int rs_check_map(const std::vector<int>& G, int k, int m, const std::vector<int>& missing,
                 FragmentMap& out)
{
    Availability av;
    if (!availability(k, m, missing, av)) return -1;
    std::vector<int> inv;
    if (!decode_inverse(G, k, av.first_k, inv)) return -1;
    const GF16& gf = GF16::get();
    out = FragmentMap();
    out.inputs = av.first_k;
    for (int f = 0; f < k + m; f++) {
        if (av.missing[f] || std::find(av.first_k.begin(), av.first_k.end(), f) != av.first_k.end()) continue;
        out.outputs.push_back(f);
        for (int c = 0; c < k; c++) {
            int v = 0;
            for (int d = 0; d < k; d++) v ^= gf.mul(G[f * k + d], inv[d * k + c]);
            out.coeff.push_back(v);
        }
    }
    return 0;
}

int rs_locate_map(const std::vector<int>& G, int k, int m, const std::vector<int>& missing,
                  FragmentMap& out, std::vector<int>& ratio)
{
    ratio.clear();
    if (rs_check_map(G, k, m, missing, out) != 0) return -1;
    const int R = static_cast<int>(out.outputs.size());
    const GF16& gf = GF16::get();
    for (int r = 1; r < R; r++)
        for (int j = 0; j < k; j++) {
            const int a0 = out.coeff[static_cast<size_t>(j)];
            if (a0 == 0) return -1;  // (never for this code: every entry of a check map is non-zero)
            ratio.push_back(gf.mul(out.coeff[static_cast<size_t>(r) * k + j], gf.inv(a0)));
        }
    return 0;
}

namespace {

// The first two rows (p < q, p ascending, then q) whose 2 x 2 minor of columns ca, cb (R entries each)
// is non-singular, and that minor's determinant; 0 for dependent columns.  Both the pair plan and the
// correction plan take their pivots from here, so they describe one minor.
int pair_minor(const int* ca, const int* cb, int R, int& p, int& q)
{
    const GF16& gf = GF16::get();
    for (p = 0; p < R; p++)
        for (q = p + 1; q < R; q++) {
            const int det = gf.mul(ca[p], cb[q]) ^ gf.mul(ca[q], cb[p]);
            if (det) return det;
        }
    return 0;
}

// Column c of [A | I] at col[c*R..].
std::vector<int> syndrome_columns(const std::vector<int>& coeff, int R, int K)
{
    const int P = K + R;
    std::vector<int> col(static_cast<size_t>(P) * R, 0);
    for (int c = 0; c < P; c++)
        for (int r = 0; r < R; r++)
            col[static_cast<size_t>(c) * R + r] = c < K ? coeff[static_cast<size_t>(r) * K + c] : (r == c - K);
    return col;
}

}  // namespace

PairPlan rs_locate_pairs_plan(const std::vector<int>& coeff, int R, int K)
{
    PairPlan out;
    out.K = K;
    out.R = R;
    if (R < 4 || K <= 0 || coeff.size() != static_cast<size_t>(R) * K) return out;
    const GF16& gf = GF16::get();
    const int P = K + R;
    const std::vector<int> col = syndrome_columns(coeff, R, K);
    out.pairs = P * (P - 1) / 2;
    out.pivot.assign(static_cast<size_t>(out.pairs) * 2, -1);
    out.L.assign(static_cast<size_t>(out.pairs) * R * 2, 0);
    int i = 0;
    for (int a = 0; a < P; a++)
        for (int b = a + 1; b < P; b++, i++) {
            const int* ca = &col[static_cast<size_t>(a) * R];
            const int* cb = &col[static_cast<size_t>(b) * R];
            int p = 0, q = 0;
            const int det = pair_minor(ca, cb, R, p, q);
            if (!det) continue;  // dependent columns: never
            out.pivot[static_cast<size_t>(i) * 2] = p;
            out.pivot[static_cast<size_t>(i) * 2 + 1] = q;
            // (S_p, S_q) = M (x, y) with M = [ca_p cb_p; ca_q cb_q]; S_r = (ca_r, cb_r) inv(M) (S_p, S_q)
            const int di = gf.inv(det);
            for (int r = 0; r < R; r++) {
                int* l = &out.L[(static_cast<size_t>(i) * R + r) * 2];
                l[0] = gf.mul(gf.mul(ca[r], cb[q]) ^ gf.mul(cb[r], ca[q]), di);
                l[1] = gf.mul(gf.mul(ca[r], cb[p]) ^ gf.mul(cb[r], ca[p]), di);
            }
        }
    // any four columns independent: eliminate each 4-subset's R x 4 matrix column by column
    out.independent4 = true;
    int sel[4];
    for (sel[0] = 0; sel[0] < P && out.independent4; sel[0]++)
        for (sel[1] = sel[0] + 1; sel[1] < P && out.independent4; sel[1]++)
            for (sel[2] = sel[1] + 1; sel[2] < P && out.independent4; sel[2]++)
                for (sel[3] = sel[2] + 1; sel[3] < P && out.independent4; sel[3]++) {
                    int v[4][32];
                    for (int c = 0; c < 4; c++)
                        for (int r = 0; r < R; r++) v[c][r] = col[static_cast<size_t>(sel[c]) * R + r];
                    bool used[32] = {false};
                    for (int c = 0; c < 4 && out.independent4; c++) {
                        int pr = -1;
                        for (int r = 0; r < R && pr < 0; r++)
                            if (!used[r] && v[c][r]) pr = r;
                        if (pr < 0) {
                            out.independent4 = false;
                            break;
                        }
                        used[pr] = true;
                        const int inv = gf.inv(v[c][pr]);
                        for (int d = c + 1; d < 4; d++) {
                            const int f = gf.mul(v[d][pr], inv);
                            if (!f) continue;
                            for (int r = 0; r < R; r++) v[d][r] ^= gf.mul(f, v[c][r]);
                        }
                    }
                }
    return out;
}

CorrectPlan rs_correct_plan(const std::vector<int>& coeff, int R, int K)
{
    CorrectPlan out;
    out.K = K;
    out.R = R;
    if (K <= 0 || R < 0 || coeff.size() != static_cast<size_t>(R) * K) return out;
    const GF16& gf = GF16::get();
    const int P = K + R;
    const std::vector<int> col = syndrome_columns(coeff, R, K);
    out.pivot.assign(static_cast<size_t>(P), -1);
    out.scale.assign(static_cast<size_t>(P), 0);
    for (int c = 0; c < P && R > 0; c++) {
        const int* cc = &col[static_cast<size_t>(c) * R];
        int p = c < K ? 0 : c - K;
        // (every entry of a check map of this code is non-zero; a zero takes the first row that is not)
        for (int r = 0; r < R && !cc[p]; r++)
            if (cc[r]) p = r;
        if (!cc[p]) continue;
        out.pivot[static_cast<size_t>(c)] = p;
        out.scale[static_cast<size_t>(c)] = gf.inv(cc[p]);
    }
    if (R < 2) return out;
    out.pairs = P * (P - 1) / 2;
    out.pair_pivot.assign(static_cast<size_t>(out.pairs) * 2, -1);
    out.minv.assign(static_cast<size_t>(out.pairs) * 4, 0);
    int i = 0;
    for (int a = 0; a < P; a++)
        for (int b = a + 1; b < P; b++, i++) {
            const int* ca = &col[static_cast<size_t>(a) * R];
            const int* cb = &col[static_cast<size_t>(b) * R];
            int p = 0, q = 0;
            const int det = pair_minor(ca, cb, R, p, q);
            if (!det) continue;
            out.pair_pivot[static_cast<size_t>(i) * 2] = p;
            out.pair_pivot[static_cast<size_t>(i) * 2 + 1] = q;
            // M = [ca_p cb_p; ca_q cb_q]; in characteristic 2 inv(M) = [cb_q cb_p; ca_q ca_p] / det
            const int di = gf.inv(det);
            int* w = &out.minv[static_cast<size_t>(i) * 4];
            w[0] = gf.mul(cb[q], di);
            w[1] = gf.mul(cb[p], di);
            w[2] = gf.mul(ca[q], di);
            w[3] = gf.mul(ca[p], di);
        }
    return out;
}

}  // namespace ecamd
