// gf16.hpp -- GF(2^16) host arithmetic and Reed-Solomon (systematic Vandermonde) planning.
//
// MI355X design note: all of this runs once per (k,m) or per erasure pattern on the host
// (k <= 255, so at most a 255x255 inversion); the per-byte work runs on the GPU through the
// split-table kernels in ../hip/ecamd_kernels.hip, fed by the tables built in tables.cpp.
//
// Semantics follow the reference built-in codec:
//   field: log/antilog over x^16+x^12+x^3+x+1 ........ src/builtin/rs_vand/rs_galois.c:38-117
//   generator: Vandermonde rows r^c, column-reduced to a systematic form, parity columns
//              normalised so the first parity row is all ones
//                                                      src/builtin/rs_vand/liberasurecode_rs_vand.c:139-289
//   inversion: Gauss-Jordan .......................... liberasurecode_rs_vand.c:293-334
//   decode / reconstruct coefficient rows ............ liberasurecode_rs_vand.c:412-558
#pragma once
#include <cstdint>
#include <vector>

namespace ecamd {

class GF16 {
public:
    static const GF16& get();
    int mul(int a, int b) const
    {
        if (a == 0 || b == 0) return 0;
        return exp_[log_[a] + log_[b]];
    }
    int inv(int a) const { return a == 0 ? -1 : exp_[kOrder - log_[a]]; }
    int log(int a) const { return log_[a]; }
    static constexpr int kPoly = 0x1100b;
    static constexpr int kOrder = 65535;

private:
    GF16();
    std::vector<int> log_;
    std::vector<int> exp_;  // 2*order entries, so log sums need no reduction
};

// (k+m) x k row-major systematic generator; empty on failure.
std::vector<int> rs_generator(int k, int m);

// Inverse of the n x n matrix a; returns false if singular.
bool gf16_invert(std::vector<int> a, std::vector<int>& inv, int n);

// A linear "fragment map": outputs[r] = sum_j coeff[r*K + j] * inputs[j].
struct FragmentMap {
    std::vector<int> inputs;   // fragment indices read (K of them)
    std::vector<int> outputs;  // fragment indices written (R of them)
    std::vector<int> coeff;    // R x K
};

// Decode map (liberasurecode_rs_vand_decode): first k available fragments in index order as
// inputs; every missing data fragment (inverse rows) and, if rebuild_parity, every missing
// parity fragment (generator row composed with the inverse) as outputs, in index order.
// Returns 0, or -1 when more than m fragments are missing.
int rs_decode_map(const std::vector<int>& G, int k, int m, const std::vector<int>& missing,
                  bool rebuild_parity, FragmentMap& out);

// Reconstruct map for one destination (liberasurecode_rs_vand_reconstruct).
int rs_reconstruct_map(const std::vector<int>& G, int k, int m, const std::vector<int>& missing,
                       int dest, FragmentMap& out);

// Check map (ecamd_rs_check): the first k available fragments as inputs, every OTHER available
// fragment as an output, ascending; row f = G[f] * inv(G[inputs]) is the value the inputs imply for
// fragment f (nothing missing: the generator's parity rows, the encode map).  Returns 0, or -1 when
// more than m fragments are missing; with exactly m missing there are no outputs.
int rs_check_map(const std::vector<int>& G, int k, int m, const std::vector<int>& missing,
                 FragmentMap& out);

// Locate map (ecamd_rs_locate): the check map, and ratio[(R - 1) * k] with ratio[(r - 1) * k + j] =
// coeff[r][j] / coeff[0][j] over its R rows (empty for R < 2).  One bad input j makes every word's
// syndrome S_r = coeff[r][j] * e, so S_r == ratio[r][j] * S_0 names it.  Returns as rs_check_map.
int rs_locate_map(const std::vector<int>& G, int k, int m, const std::vector<int>& missing,
                  FragmentMap& out, std::vector<int>& ratio);

// Pair plan (ecamd_rs_locate_pairs): which TWO participants of a check map explain a syndrome.  The
// participants are the K inputs (0..K-1), then the R checked rows (K..K+R-1); participant c has column
// c of the R x (K+R) syndrome matrix [A | I].  Pair i of a < b, in the order (0,1), (0,2), ...,
// (K+R-2, K+R-1): pivot[2i..] = two rows (p, q) whose 2 x 2 minor of columns a, b is non-singular, and
// L[(i*R + r)*2..] with S_r == L[r][0]*S_p ^ L[r][1]*S_q for every row r exactly when the syndrome S lies
// in the span of the two columns (rows p and q of L are (1,0) and (0,1)).  A pair of dependent columns
// has pivot (-1, -1) and zero L rows: it is never tested.  independent4: any four columns of [A | I] are
// linearly independent, so a syndrome that needs two columns lies in the span of no other pair (at
// most C(K+R, 4) rank computations).  Empty (pairs 0) for R < 4.
struct PairPlan {
    int K = 0, R = 0, pairs = 0;
    bool independent4 = false;
    std::vector<int> pivot;  // pairs x 2
    std::vector<int> L;      // pairs x R x 2
};
PairPlan rs_locate_pairs_plan(const std::vector<int>& coeff, int R, int K);

// Correction plan (ecamd_rs_correct): the error VALUE of a located fragment, from one or two syndrome
// rows.  Participants as in the pair plan.  Participant c: pivot[c] = a row where column c of [A | I] is
// non-zero (row 0 for an input, its own row for a checked fragment) and scale[c] = the inverse of that
// entry (1 for a checked fragment), so that a stripe whose only bad fragment is c has the error
// e_c = scale[c] * S_pivot[c] in every word.  Pair i of a < b, in the pair plan's order, for R >= 2:
// pair_pivot[2i..] = the rows (p, q) rs_locate_pairs_plan picks (the same search) and minv[4i..] the
// row-major inverse of the 2 x 2 minor of columns a, b at those rows:
//     e_a = minv[0]*S_p ^ minv[1]*S_q,   e_b = minv[2]*S_p ^ minv[3]*S_q.
// Dependent columns: pivots (-1, -1), minv zero.  R < 2: pairs 0.  R == 0: pivots -1, scales 0.
struct CorrectPlan {
    int K = 0, R = 0, pairs = 0;
    std::vector<int> pivot, scale;  // K + R each
    std::vector<int> pair_pivot;    // pairs x 2
    std::vector<int> minv;          // pairs x 4
};
CorrectPlan rs_correct_plan(const std::vector<int>& coeff, int R, int K);

// Encode map: inputs 0..k-1, outputs k..k+m-1, generator parity rows.
FragmentMap rs_encode_map(const std::vector<int>& G, int k, int m);

}  // namespace ecamd
