"""CPU: planning of the on-device correction (ecamd_rs_correct_map, include/ecamd_host.h) and the rule
it serves.  The plan's pivots, scales and 2 x 2 inverses are checked against plain numpy GF(2^16)
(gfnp) and against the pair plan's pivots; a numpy model of the rule -- error value = plan constants
times one or two syndromes -- is run on stripes of the reference encode (oracle_lib) with injected
errors and must give back exactly the injected values."""
import ctypes as C
import itertools

import numpy as np
import pytest

import gfnp
import oracle_lib as orc
from liberasurecode_amd import _lib
from test_check_planning import stripe
from test_locate_pairs_planning import MAXP, MAXPAIRS, columns, pairs_map, vmul
from test_locate_planning import gf_mul, syndromes

CASES = [(10, 4, []), (10, 4, [2]), (10, 4, [0, 11]), (4, 2, []), (20, 8, []), (20, 8, [2]), (20, 8, [0, 11]),
         (20, 8, [3, 25])]


def correct_map(k, m, missing, with_pairs=True):
    """(rc, inputs, checked, rows, pivot, scale, pair_pivots, minv): pivot / scale per participant,
    pair_pivots[i] = (p, q) and minv[i] = (m0, m1, m2, m3) for pair i in the order (0,1), (0,2), ..."""
    h = _lib.host()
    G = _lib.ints(orc.generator(k, m))
    inputs = (C.c_int * k)()
    checked = (C.c_int * (k + m))()
    coeff = (C.c_int * ((k + m) * k))()
    pivot = (C.c_int * (MAXP + 8))(*([-9] * (MAXP + 8)))
    scale = (C.c_int * (MAXP + 8))(*([-9] * (MAXP + 8)))
    pp = (C.c_int * (MAXPAIRS * 2 + 8))(*([-9] * (MAXPAIRS * 2 + 8)))
    mi = (C.c_int * (MAXPAIRS * 4 + 8))(*([-9] * (MAXPAIRS * 4 + 8)))
    n, npairs = C.c_int(-7), C.c_int(-7)
    rc = h.ecamd_rs_correct_map(G, k, m, _lib.ints(list(missing) + [-1]), inputs, checked, coeff, C.byref(n), pivot, scale,
                                C.byref(npairs) if with_pairs else None, pp if with_pairs else None,
                                mi if with_pairs else None)
    if rc != 0:
        return rc, None, None, None, None, None, None, None
    R = n.value
    P = k + R
    N = npairs.value if with_pairs else 0
    rows = [[coeff[r * k + j] for j in range(k)] for r in range(R)]
    # nothing past the plan is written
    assert all(v == -9 for v in pivot[P:P + 8]) and all(v == -9 for v in scale[P:P + 8])
    assert all(v == -9 for v in pp[2 * N:2 * N + 8]) and all(v == -9 for v in mi[4 * N:4 * N + 8])
    return (rc, list(inputs), list(checked[:R]), rows, list(pivot[:P]), list(scale[:P]),
            [(pp[2 * i], pp[2 * i + 1]) for i in range(N)], [tuple(mi[4 * i:4 * i + 4]) for i in range(N)])


@pytest.mark.parametrize("k,m,missing", CASES)
def test_pivots_scales_and_inverses(k, m, missing):
    rc, inputs, checked, rows, pivot, scale, pp, minv = correct_map(k, m, missing)
    avail = [f for f in range(k + m) if f not in missing]
    assert rc == 0 and inputs == avail[:k] and checked == avail[k:]
    R, P = len(rows), k + len(rows)
    cols = columns(rows)
    for c in range(P):
        assert pivot[c] == (0 if c < k else c - k)
        assert gf_mul(scale[c], cols[c][pivot[c]]) == 1, (missing, c)
        if c >= k:
            assert scale[c] == 1
    assert len(pp) == P * (P - 1) // 2  # R >= 2 in every case
    for i, (a, b) in enumerate(itertools.combinations(range(P), 2)):
        p, q = pp[i]
        assert 0 <= p < q < R, (missing, a, b)
        M = ((cols[a][p], cols[b][p]), (cols[a][q], cols[b][q]))
        w = minv[i]
        prod = [[gf_mul(w[2 * r], M[0][c]) ^ gf_mul(w[2 * r + 1], M[1][c]) for c in range(2)] for r in range(2)]
        assert prod == [[1, 0], [0, 1]], (missing, a, b)
    if R >= 4:  # one minor for both plans
        assert pp == pairs_map(k, m, missing)[4]


def test_pair_arrays_may_be_null_and_too_many_missing_is_refused():
    for k, m, missing in ((10, 4, []), (20, 8, [3, 25]), (4, 2, [])):
        full = correct_map(k, m, missing)
        single = correct_map(k, m, missing, with_pairs=False)
        assert single[0] == 0 and single[1:6] == full[1:6] and single[6] == [] and single[7] == []
    assert correct_map(10, 4, [0, 1, 2, 3, 4])[0] == -1
    assert correct_map(4, 2, [0, 1, 5])[0] == -1
    assert correct_map(20, 8, list(range(9)), with_pairs=False)[0] == -1


def test_fewer_than_two_checked_fragments_have_no_pairs():
    rc, _, checked, rows, pivot, scale, pp, _ = correct_map(10, 4, [1, 5, 12])
    assert rc == 0 and len(checked) == 1 and pp == []
    assert pivot == [0] * 11 and all(gf_mul(scale[c], columns(rows)[c][0]) == 1 for c in range(11))
    rc, _, checked, _, pivot, scale, pp, _ = correct_map(4, 2, [0, 3])
    assert rc == 0 and checked == [] and pp == [] and pivot == [-1] * 4 and scale == [0] * 4


# ---- the rule, as a numpy model ---------------------------------------------------------------

W = 64


def good_words(k, m, missing, seed):
    _, inputs, checked, rows, pivot, scale, pp, minv = correct_map(k, m, missing)
    full = stripe(k, m, 2 * W, seed)
    words = np.stack([full[f].view("<u2") for f in inputs + checked]).copy()
    assert not syndromes(rows, words).any()
    return rows, pivot, scale, pp, minv, words


def inject(words, where, rng):
    """XOR a random non-zero error into word w of participant c for every (c, w); the error array."""
    err = np.zeros_like(words)
    for c, w in where:
        err[c, w] = np.uint16(rng.integers(1, 65536))
    return err


@pytest.mark.parametrize("k,m,missing", CASES)
def test_model_recovers_every_single_error_value(k, m, missing):
    rows, pivot, scale, _, _, words = good_words(k, m, missing, 300 + k)
    rng = np.random.default_rng(21)
    for c in range(len(words)):
        w0, w1 = rng.choice(W, 2, replace=False)
        err = inject(words, [(c, w0), (c, w1)], rng)
        S = syndromes(rows, words ^ err)
        got = gfnp.mul_vec(scale[c], S[pivot[c]])
        assert np.array_equal(got, err[c]), (missing, c)


def pair_cases(k, m, missing, rng):
    rows = correct_map(k, m, missing)[3]
    P = k + len(rows)
    allp = list(itertools.combinations(range(P), 2))
    if (k, m) == (20, 8):
        return [allp[i] for i in rng.choice(len(allp), 60, replace=False)]
    return allp


@pytest.mark.parametrize("k,m,missing", [(10, 4, []), (10, 4, [2]), (20, 8, []), (20, 8, [3, 25]), (4, 2, [])])
def test_model_recovers_both_error_values_of_a_pair(k, m, missing):
    rows, _, _, pp, minv, words = good_words(k, m, missing, 400 + k)
    P = len(words)
    index = {ab: i for i, ab in enumerate(itertools.combinations(range(P), 2))}
    rng = np.random.default_rng(22)
    for a, b in pair_cases(k, m, missing, rng):
        i = index[(a, b)]
        p, q = pp[i]
        for same in (True, False):
            wa = int(rng.integers(0, W))
            wb = wa if same else (wa + 1 + int(rng.integers(0, W - 1))) % W
            err = inject(words, [(a, wa), (b, wb)], rng)
            S = syndromes(rows, words ^ err).astype(np.int64)
            ea = vmul(minv[i][0], S[p]) ^ vmul(minv[i][1], S[q])
            eb = vmul(minv[i][2], S[p]) ^ vmul(minv[i][3], S[q])
            assert np.array_equal(ea, err[a]) and np.array_equal(eb, err[b]), (missing, a, b, same)
