"""CPU: planning of the pair locate (ecamd_rs_locate_pairs_map, include/ecamd_host.h) and the rule it
serves.  The plan's pivots and L rows are checked against plain numpy GF(2^16) (gfnp), the four-column
independence flag against a numpy rank test, and a numpy model of the device rule is run on stripes of
the reference encode (oracle_lib) whose damaged pair is known by construction."""
import ctypes as C
import itertools

import numpy as np
import pytest

import gfnp
import oracle_lib as orc
from liberasurecode_amd import _lib
from test_check_planning import patterns, stripe
from test_locate_planning import gf_inv, gf_mul, syndromes

CODES = [(10, 4), (8, 4), (12, 6), (20, 8)]
MAXP = 32
MAXPAIRS = MAXP * (MAXP - 1) // 2


def pairs_map(k, m, missing, G=None):
    """(rc, inputs, checked, rows, pivots, L, independent4): pivots[i] = (p, q), L[i][r] = (l0, l1) for
    pair i of the participants in the order (0,1), (0,2), ..."""
    h = _lib.host()
    G = _lib.ints(orc.generator(k, m) if G is None else G)
    inputs = (C.c_int * k)()
    checked = (C.c_int * (k + m))()
    coeff = (C.c_int * ((k + m) * k))()
    pivots = (C.c_int * (MAXPAIRS * 2))(*([-9] * (MAXPAIRS * 2)))
    L = (C.c_int * (MAXPAIRS * MAXP * 2))(*([-9] * (MAXPAIRS * MAXP * 2)))
    n, npairs, ind = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    rc = h.ecamd_rs_locate_pairs_map(G, k, m, _lib.ints(list(missing) + [-1]), inputs, checked, coeff, C.byref(n),
                                     C.byref(npairs), pivots, L, C.byref(ind))
    if rc != 0:
        return rc, None, None, None, None, None, None
    R, N = n.value, npairs.value
    rows = [[coeff[r * k + j] for j in range(k)] for r in range(R)]
    piv = [(pivots[2 * i], pivots[2 * i + 1]) for i in range(N)]
    Ls = [[(L[(i * R + r) * 2], L[(i * R + r) * 2 + 1]) for r in range(R)] for i in range(N)]
    # nothing past the plan is written
    assert all(v == -9 for v in pivots[2 * N:2 * N + 8]) and all(v == -9 for v in L[2 * N * R:2 * N * R + 8])
    return rc, list(inputs), list(checked[:R]), rows, piv, Ls, ind.value


def columns(rows):
    """Column c of [A | I] for participant c (inputs, then checked rows)."""
    R, K = len(rows), len(rows[0])
    return [[rows[r][c] for r in range(R)] for c in range(K)] + [[int(r == c) for r in range(R)] for c in range(R)]


def big_patterns(k, m):
    return [missing for missing, ncheck in patterns(k, m) if ncheck is not None and ncheck >= 4]


def vmul(a, b):
    """Elementwise GF(2^16) product of two integer arrays."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    out = gfnp.EXP[gfnp.LOG[a] + gfnp.LOG[b]]
    return np.where((a == 0) | (b == 0), 0, out)


def vinv(a):
    a = np.asarray(a, np.int64)
    return gfnp.EXP[(65535 - gfnp.LOG[a]) % 65535]


def any_four_columns_independent(cols):
    """Rank test of every 4-subset of the columns by elimination in numpy, all subsets at once."""
    cols = np.array(cols, np.int64)  # P x R
    sel = np.array(list(itertools.combinations(range(len(cols)), 4)))
    V = cols[sel]  # N x 4 x R
    N, _, R = V.shape
    used = np.zeros((N, R), bool)
    ok = np.ones(N, bool)
    idx = np.arange(N)
    for c in range(4):
        cand = (V[:, c, :] != 0) & ~used
        ok &= cand.any(axis=1)
        pr = cand.argmax(axis=1)
        used[idx, pr] = True
        pv = V[idx, c, pr]
        inv = vinv(np.where(pv == 0, 1, pv))
        for d in range(c + 1, 4):
            f = vmul(V[idx, d, pr], inv)
            V[:, d, :] ^= vmul(f[:, None], V[:, c, :])
    return bool(ok.all())


@pytest.mark.parametrize("k,m", CODES)
def test_pivots_and_L_rows(k, m):
    for missing in big_patterns(k, m):
        rc, inputs, checked, rows, piv, Ls, ind = pairs_map(k, m, missing)
        avail = [f for f in range(k + m) if f not in missing]
        assert rc == 0 and inputs == avail[:k] and checked == avail[k:]
        R, P = len(rows), k + len(rows)
        cols = columns(rows)
        assert len(piv) == P * (P - 1) // 2
        for i, (a, b) in enumerate(itertools.combinations(range(P), 2)):
            p, q = piv[i]
            assert 0 <= p < q < R, (missing, a, b)
            det = gf_mul(cols[a][p], cols[b][q]) ^ gf_mul(cols[a][q], cols[b][p])
            assert det != 0, (missing, a, b)
            for col in (cols[a], cols[b]):  # L . col[pivots] == col
                for r in range(R):
                    assert gf_mul(Ls[i][r][0], col[p]) ^ gf_mul(Ls[i][r][1], col[q]) == col[r], (missing, a, b, r)
            assert Ls[i][p] == (1, 0) and Ls[i][q] == (0, 1)


@pytest.mark.parametrize("k,m", CODES)
def test_independence_flag_equals_a_numpy_rank_test(k, m):
    for missing in big_patterns(k, m):
        _, _, _, rows, _, _, ind = pairs_map(k, m, missing)
        assert ind == int(any_four_columns_independent(columns(rows))) == 1, missing


def test_dependent_columns_clear_the_flag_and_get_the_never_marker():
    k, m = 10, 4
    G = list(orc.generator(k, m))
    for p in range(m):  # input 1 enters every parity as input 0 does
        G[(k + p) * k + 1] = G[(k + p) * k]
    rc, _, _, rows, piv, Ls, ind = pairs_map(k, m, [], G)
    assert rc == 0 and ind == 0 == int(any_four_columns_independent(columns(rows)))
    assert piv[0] == (-1, -1) and all(l == (0, 0) for l in Ls[0])
    assert all(p >= 0 for p, _ in piv[1:])
    # three columns in one plane: pairs are fine, the flag is not
    G = list(orc.generator(k, m))
    for p in range(m):
        G[(k + p) * k + 2] = G[(k + p) * k] ^ G[(k + p) * k + 1]
    rc, _, _, rows, piv, _, ind = pairs_map(k, m, [], G)
    assert rc == 0 and ind == 0 == int(any_four_columns_independent(columns(rows)))
    assert all(p >= 0 for p, _ in piv)


def test_fewer_than_four_checked_fragments_yield_no_plan():
    for k, m, missing in ((10, 4, [0]), (10, 4, [2, 7]), (4, 2, []), (10, 4, [0, 1, 2, 3]), (12, 6, [0, 1, 2])):
        rc, inputs, checked, rows, piv, Ls, ind = pairs_map(k, m, missing)
        assert rc == 0 and len(checked) == m - len(missing) and piv == [] and Ls == [] and ind == 0
    assert pairs_map(10, 4, [0, 1, 2, 3, 4])[0] == -1


# ---- the rule, as a numpy model ---------------------------------------------------------------

def single_explains(col, S):
    """Per word: the syndrome is a multiple of the column."""
    p = next(r for r, c in enumerate(col) if c)
    ok = np.ones(S.shape[1], bool)
    for r, c in enumerate(col):
        ok &= gfnp.mul_vec(gf_mul(c, gf_inv(col[p])), S[p]) == S[r]
    return ok


def pairs_explain(piv, Ls, S):
    """Per pair and word: S_r == L[r][0] S_p ^ L[r][1] S_q for every row."""
    piv, L, S = np.array(piv), np.array(Ls, np.int64), S.astype(np.int64)
    Sp, Sq = S[piv[:, 0]], S[piv[:, 1]]
    ok = np.ones(Sp.shape, bool)
    for r in range(S.shape[0]):
        ok &= (vmul(L[:, r, 0][:, None], Sp) ^ vmul(L[:, r, 1][:, None], Sq)) == S[r][None, :]
    return ok


def model(rows, piv, Ls, S):
    """(the device rule's word, the set of pairs that explain every dirty word).  The rule ORs per
    dirty word: the single participant that explains it, else the first pair that does, else all
    ones; a word of exactly two bits is the answer."""
    P = len(rows[0]) + len(rows)
    cols = columns(rows)
    dirty = S.any(axis=0)
    singles = [single_explains(cols[c], S) for c in range(P)]
    pairs = list(itertools.combinations(range(P), 2))
    pok = pairs_explain(piv, Ls, S)
    word = 0
    for w in np.nonzero(dirty)[0]:
        one = [c for c in range(P) if singles[c][w]]
        two = [pairs[i] for i in range(len(pairs)) if pok[i][w]]
        if one:
            word |= 1 << one[0]
        elif two:
            word |= (1 << two[0][0]) | (1 << two[0][1])
        else:
            word |= 0xFFFFFFFF
    every = {pairs[i] for i in range(len(pairs)) if pok[i][dirty].all()}
    return (word if bin(word).count("1") == 2 else 0), every


def damaged(words, a, b, same_word, rng):
    bad = words.copy()
    wa = int(rng.integers(0, words.shape[1]))
    wb = wa if same_word else (wa + 1 + int(rng.integers(0, words.shape[1] - 1))) % words.shape[1]
    bad[a, wa] ^= np.uint16(rng.integers(1, 65536))
    bad[b, wb] ^= np.uint16(rng.integers(1, 65536))
    return bad


def test_model_names_every_pair_of_10_4():
    k, m = 10, 4
    _, inputs, checked, rows, piv, Ls, ind = pairs_map(k, m, [])
    assert ind == 1
    full = stripe(k, m, 64, 123)
    words = np.stack([full[f].view("<u2") for f in inputs + checked]).copy()
    rng = np.random.default_rng(11)
    for a, b in itertools.combinations(range(k + m), 2):
        for same in (True, False):
            word, every = model(rows, piv, Ls, syndromes(rows, damaged(words, a, b, same, rng)))
            assert every == {(a, b)}, (a, b, same, every)
            assert word == (1 << a) | (1 << b), (a, b, same, hex(word))


def test_model_names_pairs_of_20_8_and_no_pair_for_three_errors():
    k, m = 20, 8
    rng = np.random.default_rng(12)
    full = stripe(k, m, 64, 124)
    for missing in ([], [2, 7]):
        _, inputs, checked, rows, piv, Ls, ind = pairs_map(k, m, missing)
        assert ind == 1
        P = k + len(rows)
        words = np.stack([full[f].view("<u2") for f in inputs + checked]).copy()
        allp = list(itertools.combinations(range(P), 2))
        sample = [allp[i] for i in rng.choice(len(allp), 24, replace=False)] + [(0, 1), (P - 2, P - 1), (k - 1, k)]
        for n, (a, b) in enumerate(sample):
            word, every = model(rows, piv, Ls, syndromes(rows, damaged(words, a, b, n % 2 == 0, rng)))
            assert every == {(a, b)}, (missing, a, b, every)
            assert word == (1 << a) | (1 << b), (missing, a, b, hex(word))
        for _ in range(20):  # three errors in one word: five independent columns leave no pair
            a, b, c = sorted(rng.choice(P, 3, replace=False))
            bad = words.copy()
            for f in (a, b, c):
                bad[f, 9] ^= np.uint16(rng.integers(1, 65536))
            word, every = model(rows, piv, Ls, syndromes(rows, bad))
            assert word == 0 and every == set(), (missing, a, b, c, hex(word), every)
